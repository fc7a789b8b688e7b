"""FM-index factorize / unfactorize (tc_fm_factorize, tc_fm_unfactorize and their _dev forms) against the brute-force
reference of tests/factor_ref.py: fac_offs, fac_pos and fac_len are compared exactly, on the smallest shapes at which the
kernel can go wrong (rank-line boundaries, every alphabet class, bytes the text does not hold, the length edges, a
divergent batch of more than one workgroup), through the host and the device entry points, on a full and on sampled
indexes.  What the parse does on an imported index that no build wrote is argued from the loop's bounds in DESIGN.md 5e
and tested in tests/test_gpu_fm_import_foreign.py against the model of tests/fm_wire_ref.py."""
import ctypes as C

import numpy as np
import pytest

import factor_ref as R

pytestmark = pytest.mark.gpu

SAMPLED_RATES = (4, 4096)       # 4096 exceeds every n here: every walk ends at the primary row
TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
FOREIGN = (0, 7, 255)           # byte values none of the alphabets below holds (the 256-value alphabet holds every one)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
def _text(seed, n, alphabet):
    rng = np.random.default_rng(seed)
    a = np.frombuffer(bytes(alphabet), np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def _sub(rng, tb, m):
    o = int(rng.integers(0, len(tb) - m + 1))
    return tb[o:o + m]


def _patterns(seed, tb, alphabet, max_len=None, whole=True):
    """the pattern kinds of one text; max_len caps every pattern (the 256-value alphabet)"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(bytes(alphabet), np.uint8)
    n = len(tb)
    foreign = [b for b in FOREIGN if b not in alphabet]
    cap = max_len or (1 << 30)
    lens = [m for m in (1, 2, 3, 17, 100) if m <= min(n, cap)]
    pats = [_sub(rng, tb, m) for m in lens for _ in range(2)]                       # substrings: one factor each
    top = lens[-1]
    pats.append((_sub(rng, tb, top) + _sub(rng, tb, top))[:cap])                    # two and three substrings joined
    pats.append((_sub(rng, tb, min(top, 17)) + _sub(rng, tb, 1) + _sub(rng, tb, min(top, 17)))[:cap])
    for planted in (1, 2, 4):                                                       # planted substitutions
        p = bytearray(_sub(rng, tb, top))
        for j in rng.choice(len(p), size=min(planted, len(p)), replace=False):
            p[int(j)] = int(a[rng.integers(0, len(a))])
        pats.append(bytes(p))
    if foreign:                                                                     # bytes the text does not hold
        f = bytes(foreign)
        mid = _sub(rng, tb, min(top, 17))
        pats += [f[:1] + mid, mid + f[-1:], mid + f[:1] + mid, f + mid + f + f[:1] + mid + f, f, f[:1] * 5]
    pats.append(b"")                                                                # the empty pattern
    if whole and n <= cap:
        pats += [tb, tb + tb]                                                       # the whole text, and twice over
    for m in (1, 2, 5, 33):                                                         # random strings
        pats.append(a[rng.integers(0, len(a), min(m, cap))].tobytes())
    return pats


def _dev_patterns(pats):
    import torch
    from textcomp import FMIndexHandle
    flat, offs = FMIndexHandle._pack(pats)
    return torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()


def _factorize_dev(fm, pats):
    d_flat, d_offs = _dev_patterns(pats)
    foffs, fpos, flen = fm.factorize_dev(d_flat, d_offs, len(pats))
    return foffs.cpu().numpy().astype(np.uint64), fpos.cpu().numpy().astype(np.uint64), flen.cpu().numpy().astype(np.uint32)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


def _explain(tb, pats, got, want):
    for i, p in enumerate(pats):
        g = list(zip(got[1][int(got[0][i]):int(got[0][i + 1])].tolist(), got[2][int(got[0][i]):int(got[0][i + 1])].tolist()))
        w = list(zip(want[1][int(want[0][i]):int(want[0][i + 1])].tolist(), want[2][int(want[0][i]):int(want[0][i + 1])].tolist()))
        if g != w:
            return "n=%d pattern %d %r: got %r, want %r" % (len(tb), i, p[:40], g[:8], w[:8])
    return "offsets differ"


def _four_ways(ctx, tb, pats):
    """factorize through the host and the _dev entry, on a full and on the sampled indexes: every answer equal to the
    reference as raw arrays"""
    want = R.factorize(tb, pats)
    full = ctx.fm_build(tb)
    sampled = [ctx.fm_build(tb, sa_rate=r) for r in SAMPLED_RATES]
    try:
        for fm in [full] + sampled:
            for how in (fm.factorize, lambda p, fm=fm: _factorize_dev(fm, p)):
                got = how(pats)
                assert got[0][0] == 0 and got[0][-1] == len(got[1]) == len(got[2])
                assert _same(got, want), (fm.sa_rate, _explain(tb, pats, got, want))
            assert np.array_equal(fm.factor_counts(pats), np.diff(want[0]))
    finally:
        full.close()
        for s in sampled:
            s.close()
    print("n=%d: %d patterns, %d factors, all as the reference (host and _dev; full, rate 4, rate 4096)"
          % (len(tb), len(pats), len(want[1])))


# ------------------------------------------------------------------------------------------------ 1: rank-line boundaries
@pytest.mark.parametrize("n", [446, 447, 448, 894, 895, 896])
def test_rank_line_boundaries(ctx, n):
    """FM_LINE_BITS = 448: N = n + 1 rows on either side of one and of two lines"""
    tb = _text(0x5100 + n, n, b"ACGT")
    _four_ways(ctx, tb, _patterns(0x5200 + n, tb, b"ACGT"))


# ------------------------------------------------------------------------------------------------ 2: alphabets
ALPHABETS = {1: b"A", 2: b"AC", 4: b"ACGT", 5: b"ACGNT", 6: b"ACGNTU", 256: bytes(range(256))}


@pytest.mark.parametrize("sigma", sorted(ALPHABETS))
def test_alphabets(ctx, sigma):
    """1, 2, 4, 5 byte values (pair vectors; 5 is their limit), 6 (none) and all 256 (patterns of at most 32 bytes)"""
    al = ALPHABETS[sigma]
    n = 1500 if sigma == 256 else 700
    tb = _text(0x5300 + sigma, n, al)
    _four_ways(ctx, tb, _patterns(0x5400 + sigma, tb, al, max_len=32 if sigma == 256 else None))


def test_text_of_8192_bytes(ctx):
    tb = _text(0x5500, 8192, b"ACGT")
    _four_ways(ctx, tb, _patterns(0x5501, tb, b"ACGT"))


def test_tiny_texts(ctx):
    """n = 1 and 2: no pair vectors below n = 2, and every phrase is at most the text"""
    for tb in (b"A", b"AC", b"AA"):
        _four_ways(ctx, tb, [b"A", b"C", b"AC", b"CA", b"AAAA", b"ACAC", b"", b"G", b"GAG"])


# ------------------------------------------------------------------------------------------------ 3: one divergent batch
def test_divergent_batch(ctx):
    """300 patterns of lengths 0 .. 2000 in one launch: more than one workgroup, lanes finishing far apart"""
    tb = _text(0x5600, 8192, b"ACGNT")
    rng = np.random.default_rng(0x5601)
    al = np.frombuffer(b"ACGNT", np.uint8)
    lens = [0, 2000] + [int(v) for v in rng.integers(0, 2001, 298)]
    pats = []
    for i, m in enumerate(lens):
        if i % 3 == 0 and m:                # a mosaic of substrings: long phrases
            p = b""
            while len(p) < m:
                p += _sub(rng, tb, int(rng.integers(1, 200)))
            pats.append(p[:m])
        else:                               # random: phrases of about log_5 n bytes
            pats.append(al[rng.integers(0, 5, m)].tobytes())
    _four_ways(ctx, tb, pats)


# ------------------------------------------------------------------------------------------------ 4: capacity
def _raw_factorize(fm, pats, cap, fpos, flen, dev=False):
    from textcomp import FMIndexHandle
    ctx = fm._ctx
    foffs = np.full(len(pats) + 1, 99, np.uint64)
    nf = C.c_uint64(cap)
    flat, offs = FMIndexHandle._pack(pats)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.tc_fm_factorize(ctx.handle, fm._h, p(flat), p(offs), len(pats), p(foffs), p(fpos), p(flen), C.byref(nf))
    return rc, int(nf.value), foffs


@pytest.mark.parametrize("sa_rate", [1, 4])
def test_capacity(ctx, sa_rate):
    import torch
    tb = _text(0x5700, 700, b"ACGT")
    pats = _patterns(0x5701, tb, b"ACGT")
    want = R.factorize(tb, pats)
    total = len(want[1])
    fm = ctx.fm_build(tb, sa_rate=sa_rate)
    try:
        # one short: the total, the payload untouched
        fpos, flen = np.full(total, 0x77, np.uint64), np.full(total, 0x77, np.uint32)
        rc, nf, _ = _raw_factorize(fm, pats, total - 1, fpos, flen)
        assert rc == TC_ERR_CAPACITY and nf == total
        assert (fpos == 0x77).all() and (flen == 0x77).all()
        # exactly enough
        rc, nf, foffs = _raw_factorize(fm, pats, total, fpos, flen)
        assert rc == 0 and nf == total and _same((foffs, fpos, flen), want)
        # sizes only
        rc, nf, foffs = _raw_factorize(fm, pats, 0, None, None)
        assert rc == 0 and nf == total and np.array_equal(foffs, want[0])
        # one of the two payload arrays missing, or none with a capacity: an argument error
        assert _raw_factorize(fm, pats, total, fpos, None)[0] == TC_ERR_ARG
        assert _raw_factorize(fm, pats, total, None, None)[0] == TC_ERR_ARG
        # the same on the device
        d_flat, d_offs = _dev_patterns(pats)
        d_foffs = torch.zeros(len(pats) + 1, dtype=torch.int64, device="cuda")
        d_fpos = torch.full((total,), 0x77, dtype=torch.int64, device="cuda")
        d_flen = torch.full((total,), 0x77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        def call(cap):
            nf = C.c_uint64(cap)
            rc = ctx.lib.tc_fm_factorize_dev(ctx.handle, fm._h, C.c_void_p(d_flat.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                             len(pats), C.c_void_p(d_foffs.data_ptr()), C.c_void_p(d_fpos.data_ptr()),
                                             C.c_void_p(d_flen.data_ptr()), C.byref(nf))
            return rc, int(nf.value)

        assert call(total - 1) == (TC_ERR_CAPACITY, total)
        assert bool((d_fpos == 0x77).all()) and bool((d_flen == 0x77).all())
        assert call(total) == (0, total)
        assert np.array_equal(d_fpos.cpu().numpy().astype(np.uint64), want[1])
        assert np.array_equal(d_flen.cpu().numpy().astype(np.uint32), want[2])
        assert np.array_equal(d_foffs.cpu().numpy().astype(np.uint64), want[0])
    finally:
        fm.close()


# ------------------------------------------------------------------------------------------------ 5: round trip
@pytest.mark.parametrize("sa_rate", [1, 4])
@pytest.mark.parametrize("text_rate", [1, 4, 32])
def test_round_trip(ctx, sa_rate, text_rate):
    """unfactorize(factorize(pats)) == pats, through the host and the _dev entries"""
    tb = _text(0x5800, 1000, b"ACGNT")
    pats = _patterns(0x5801 + text_rate, tb, b"ACGNT")
    fm = ctx.fm_build(tb, sa_rate=sa_rate, text_rate=text_rate)
    try:
        fac = fm.factorize(pats)
        assert _same(fac, R.factorize(tb, pats))
        assert fm.unfactorize(*fac) == pats
        d_flat, d_offs = _dev_patterns(pats)
        d_fac = fm.factorize_dev(d_flat, d_offs, len(pats))
        offs, out = fm.unfactorize_dev(d_fac[0], d_fac[1], d_fac[2], len(pats))
        blob, offs = out.cpu().numpy().tobytes(), offs.cpu().numpy()
        assert [blob[int(offs[i]):int(offs[i + 1])] for i in range(len(pats))] == pats
    finally:
        fm.close()


def _raw_unfactorize(fm, fo, fp, fl, cap, out):
    ctx = fm._ctx
    fo, fp, fl = np.asarray(fo, np.uint64), np.asarray(fp, np.uint64), np.asarray(fl, np.uint32)
    offs = np.full(len(fo), 99, np.uint64)
    nb = C.c_uint64(cap)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.tc_fm_unfactorize(ctx.handle, fm._h, p(fo), p(fp), p(fl), len(fo) - 1, p(offs), p(out), C.byref(nb))
    return rc, int(nb.value), offs


def test_unfactorize_hand_made_and_bad_lists(ctx):
    n = 900
    tb = _text(0x5900, n, b"ACGT")
    fm = ctx.fm_build(tb, text_rate=4)
    try:
        # overlapping ranges, a range that ends at n, literals at both ends, a pattern with no factors
        fo = [0, 4, 4, 7, 8]
        fp = [0, 10, 12, 255, 5, n - 40, 200, n]
        fl = [0, 30, 30, 0, 3, 41, 0, 1]
        want = R.unfactorize(tb, fo, fp, fl)
        assert fm.unfactorize(fo, fp, fl) == want and want[1] == b"" and want[2].endswith(tb[-41:] + b"\xc8")
        total = sum(len(w) for w in want)
        out = np.full(total, 0x77, np.uint8)
        rc, nb, _ = _raw_unfactorize(fm, fo, fp, fl, total - 1, out)
        assert rc == TC_ERR_CAPACITY and nb == total and (out == 0x77).all()
        rc, nb, offs = _raw_unfactorize(fm, fo, fp, fl, total, out)
        assert rc == 0 and nb == total and out.tobytes() == b"".join(want)
        assert offs.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
        # each kind of bad list: TC_ERR_ARG, out untouched
        bad = {
            "fac_offs[0] != 0": ([1, 4, 4, 7, 8], fp, fl),
            "fac_offs decreases": ([0, 4, 3, 7, 8], fp, fl),
            "a match at pos 0": (fo, [0, 0, 12, 255, 5, n - 40, 200, n], fl),
            "a match over the end": (fo, [0, 10, 12, 255, 5, n - 39, 200, n], fl),
            "a match behind the end": (fo, [0, 10, 12, 255, 5, n - 40, 200, n + 1], fl),
            "a literal above 255": (fo, [256, 10, 12, 255, 5, n - 40, 200, n], fl),
        }
        for what, (o, a, l) in bad.items():
            out = np.full(total + 64, 0x77, np.uint8)
            rc, _, _ = _raw_unfactorize(fm, o, a, l, total + 64, out)
            assert rc == TC_ERR_ARG, what
            assert (out == 0x77).all(), what
    finally:
        fm.close()


# ------------------------------------------------------------------------------------------------ 6: edges and errors
def test_edges_and_errors(ctx):
    import textcomp
    tb = _text(0x5A00, 600, b"ACGT")
    pats = _patterns(0x5A01, tb, b"ACGT")
    want = R.factorize(tb, pats)
    # the empty index: every byte is a literal
    empty = ctx.fm_build(b"")
    try:
        got = empty.factorize([b"AC", b"", b"\x00\xff"])
        assert _same(got, (np.array([0, 2, 2, 4], np.uint64), np.array([65, 67, 0, 255], np.uint64), np.zeros(4, np.uint32)))
        assert _same(got, R.factorize(b"", [b"AC", b"", b"\x00\xff"]))
    finally:
        empty.close()
    fm = ctx.fm_build(tb, sa_rate=4, text_rate=4)
    plain = ctx.fm_build(tb)
    try:
        assert _same(fm.factorize([]), (np.zeros(1, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32)))   # npat = 0
        nf = C.c_uint64(5)
        assert ctx.lib.tc_fm_factorize(ctx.handle, fm._h, None, None, 0, None, None, None, C.byref(nf)) == 0 and nf.value == 0
        assert ctx.lib.tc_fm_factorize(ctx.handle, None, None, None, 0, None, None, None, C.byref(nf)) == TC_ERR_ARG
        assert ctx.lib.tc_fm_factorize(ctx.handle, fm._h, None, None, 3, None, None, None, C.byref(nf)) == TC_ERR_ARG
        assert ctx.lib.tc_fm_unfactorize(ctx.handle, None, None, None, None, 0, None, None, C.byref(nf)) == TC_ERR_ARG
        # unfactorize on an index without text samples
        with pytest.raises(textcomp.TcError) as ei:
            plain.unfactorize(*want)
        assert ei.value.code == TC_ERR_ARG
        # an export / import round trip with the locate part and the text samples: the same factors, and the same bytes back
        back = textcomp.FMIndexHandle.import_dev(ctx, fm.export_dev(with_locate=True), n=len(tb))
        try:
            assert _same(back.factorize(pats), want) and _same(_factorize_dev(back, pats), want)
            assert back.unfactorize(*want) == pats
        finally:
            back.close()
        # factorize on an index imported without its locate part
        bare = textcomp.FMIndexHandle.import_dev(ctx, fm.export_dev(with_locate=False), n=len(tb))
        try:
            with pytest.raises(textcomp.TcError) as ei:
                bare.factorize(pats)
            assert ei.value.code == TC_ERR_ARG
            with pytest.raises(textcomp.TcError) as ei:
                bare.unfactorize(*want)
            assert ei.value.code == TC_ERR_ARG
        finally:
            bare.close()
    finally:
        fm.close()
        plain.close()


def test_fmindex_mirrors(ctx):
    from textcomp import fmindex
    res = fmindex.bytestringFMIndexFactorizeS([b"ACGX", b""], b"TTACGTT", ctx)
    assert res == [(b"ACGX", [(3, 3), (ord("X"), 0)]), (b"", [])]
    assert fmindex.textFMIndexFactorizeP(["ACGX"], "TTACGTT", ctx) == [("ACGX", [(3, 3), (ord("X"), 0)])]
    assert fmindex.bytestringFMIndexFactorizeP([], b"TTACGTT", ctx) == []
