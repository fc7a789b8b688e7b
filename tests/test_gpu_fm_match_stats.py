"""FM-index matching statistics and maximal exact matches (tc_fm_match_stats, tc_fm_mems and their _dev forms) against the
brute-force reference of tests/ms_ref.py: ms_len, ms_pos, ms_occ and the four MEM arrays are compared exactly, on the
smallest shapes at which the kernel can go wrong (rank-line and tree-group boundaries, every alphabet class, bytes the text
does not hold, texts whose shrinks cross many groups of the min tree at the default fan-out and at fan-out 4, a divergent
batch of more than one workgroup), through the host and the _dev entry points, on a full index and on sampled ones, with
and without text samples.  Which levels of the tree the searches reach cannot be seen from here: host/check/fm_ms_kernels.cpp
(tests/test_host_checks.py) asserts that."""
import ctypes as C

import numpy as np
import pytest

import factor_ref
import ms_ref as R

pytestmark = pytest.mark.gpu

SA_RATES = (1, 4, 4096)         # 4096 exceeds every n here: every walk ends at the primary row
TEXT_RATES = (0, 4)             # without and with text samples
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
    m = min(m, len(tb))
    o = int(rng.integers(0, len(tb) - m + 1))
    return tb[o:o + m]


def _patterns(seed, tb, alphabet, max_len=None, whole=True):
    """the pattern kinds of one text (those of tests/test_gpu_fm_factorize.py); max_len caps every pattern"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(bytes(alphabet), np.uint8)
    n = len(tb)
    foreign = [b for b in FOREIGN if b not in alphabet]
    cap = max_len or (1 << 30)
    lens = [m for m in (1, 2, 3, 17, 100) if m <= min(n, cap)]
    pats = [_sub(rng, tb, m) for m in lens for _ in range(2)]                       # substrings of length 1 .. 100
    top = lens[-1]
    pats.append((_sub(rng, tb, top) + _sub(rng, tb, top))[:cap])                    # joined substrings
    pats.append((_sub(rng, tb, min(top, 17)) + _sub(rng, tb, 1) + _sub(rng, tb, min(top, 17)))[:cap])
    for planted in (1, 2, 4):                                                       # planted substitutions
        p = bytearray(_sub(rng, tb, top))
        for j in rng.choice(len(p), size=min(planted, len(p)), replace=False):
            p[int(j)] = int(a[rng.integers(0, len(a))])
        pats.append(bytes(p))
    if foreign:                                                                     # foreign bytes at either end and inside
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
    return torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), int(offs[-1])


def _np(t, dt):
    return t.cpu().numpy().astype(dt)


def _match_stats_dev(fm, pats):
    d_flat, d_offs, total = _dev_patterns(pats)
    l, p, o = fm.match_stats_dev(d_flat, d_offs, len(pats), total)
    return _np(l, np.uint32), _np(p, np.uint64), _np(o, np.uint32)


def _mems_dev(fm, pats, min_len):
    d_flat, d_offs, _ = _dev_patterns(pats)
    mo, ms, mp, ml = fm.mems_dev(d_flat, d_offs, len(pats), min_len)
    return _np(mo, np.uint64), _np(ms, np.uint64), _np(mp, np.uint64), _np(ml, np.uint32)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def _explain(pats, got, want):
    o = 0
    for j, p in enumerate(pats):
        for i in range(len(p)):
            g = tuple(int(a[o + i]) for a in got)
            w = tuple(int(a[o + i]) for a in want)
            if g != w:
                return "pattern %d %r position %d: got (len, pos, occ) = %r, want %r" % (j, p[:40], i, g, w)
        o += len(p)
    return "lengths differ"


def _set_fanout(ctx, f):
    fn = ctx.lib.tc_dbg_fm_set_lcp_fanout          # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, f)


def _indexes(ctx, tb, sa_rates=SA_RATES, text_rates=TEXT_RATES):
    return [ctx.fm_build(tb, sa_rate=r, text_rate=tr, lcp=True) for r in sa_rates for tr in text_rates]


def _every_way(ctx, tb, pats, min_lens=(1, 3), fanout=None, what=""):
    """matching statistics and MEMs through the host and the _dev entry, on a full and on the sampled indexes, with and
    without text samples: every answer equal to the reference as raw arrays"""
    ref = R.Ref(tb)
    want = ref.match_stats(pats)
    want_mems = {ml: R.mems(pats, want, ml) for ml in min_lens}
    o = 0
    for p in pats:                                  # where the enumeration is affordable the rule must equal it
        if 0 < len(p) <= 12:
            l = want[0][o:o + len(p)].tolist()
            assert [(i, l[i]) for i in R.mems_by_rule(l)] == ref.mems_enumerated(p), p
        o += len(p)
    if fanout is not None:
        assert _set_fanout(ctx, fanout) == 0
    try:
        fms = _indexes(ctx, tb)
    finally:
        if fanout is not None:
            assert _set_fanout(ctx, 64) == 0
    try:
        for fm in fms:
            assert fm.has_lcp
            for how in (fm.match_stats, lambda p, fm=fm: _match_stats_dev(fm, p)):
                got = how(pats)
                assert _same(got, want), (what, len(tb), fm.sa_rate, fm.text_rate, _explain(pats, got, want))
            for ml, wm in want_mems.items():
                for how in (fm.mems, lambda p, m, fm=fm: _mems_dev(fm, p, m)):
                    got = how(pats, ml)
                    assert _same(got, wm), (what, len(tb), fm.sa_rate, fm.text_rate, ml)
    finally:
        for fm in fms:
            fm.close()
    print("%s n=%d: %d patterns, %d positions, %s MEMs, all as the reference (host and _dev; rates %r x text rates %r)"
          % (what, len(tb), len(pats), len(want[0]), [len(w[1]) for w in want_mems.values()], SA_RATES, TEXT_RATES))
    return want


# ------------------------------------------------------------------------------------------------ 1: boundaries
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 447, 448, 449, 897])
def test_rank_line_and_tree_group_boundaries(ctx, n):
    """FM_LINE_BITS = 448 and a tree group of 64 rows: N = n + 1 rows on either side of one and of two of each"""
    al = b"AC" if n <= 2 else b"ACGT"
    tb = _text(0x6100 + n, n, al)
    _every_way(ctx, tb, _patterns(0x6200 + n, tb, al))


ALPHABETS = {1: b"A", 2: b"AC", 4: b"ACGT", 5: b"ACGNT", 96: bytes(range(32, 128)), 256: bytes(range(256))}


@pytest.mark.parametrize("sigma", sorted(ALPHABETS))
def test_alphabets(ctx, sigma):
    """1, 2, 4, 5 byte values (the index also holds pair vectors, which this search must not take), 96 and all 256"""
    al = ALPHABETS[sigma]
    n = 1500 if sigma == 256 else 449
    tb = _text(0x6300 + sigma, n, al)
    _every_way(ctx, tb, _patterns(0x6400 + sigma, tb, al, max_len=32 if sigma == 256 else None))


# ------------------------------------------------------------------------------------------------ 2: shrinks across groups
def _fibonacci(n):
    a, b = b"A", b"AB"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _shrink_texts(seed, n):
    rng = np.random.default_rng(seed)
    ab = np.frombuffer(b"AB", np.uint8)
    return {
        "unary": (b"A" * n, b"A"),
        "period 3": ((b"ACG" * (n // 3 + 1))[:n], b"ACG"),
        "fibonacci": (_fibonacci(n), b"AB"),
        "binary": (ab[rng.integers(0, 2, n)].tobytes(), b"AB"),
        "rare end": (ab[rng.integers(0, 2, n - 1)].tobytes() + b"Z", b"AB"),
    }


def _shrink_patterns(seed, kind, tb, al):
    rng = np.random.default_rng(seed)
    pats = _patterns(seed, tb, al, whole=False)
    pats.append(al[:1] * 200 + al[-1:])                                             # a long run, then one other byte
    pats.append(_sub(rng, tb, 150) + al[:1] + _sub(rng, tb, 150))
    if kind == "rare end":
        # rare + short frequent string: the step fails at depth 1 .. 3 on intervals of hundreds to thousands of rows, and
        # the one shrink widens across whole tree levels in both directions
        for w in (b"A", b"B", b"AA", b"AB", b"BA", b"BB", b"ABA", b"BBB", b"BAB"):
            pats += [b"Z" + w, w + b"Z" + w]
    return pats


@pytest.mark.parametrize("kind", ["unary", "period 3", "fibonacci", "binary", "rare end"])
@pytest.mark.parametrize("n,fanout", [(4095, None), (4096, None), (4097, None), (4161, None), (1100, 4)])
def test_shrinks_that_cross_many_groups(ctx, n, fanout, kind):
    """the default fan-out on either side of 64 groups and of 65, and fan-out 4 (five tree levels at a thousand rows)"""
    tb, al = _shrink_texts(0x6500 + n, n)[kind]
    _every_way(ctx, tb, _shrink_patterns(0x6600 + n, kind, tb, al), min_lens=(2,), fanout=fanout, what=kind)


def test_fanout_argument(ctx):
    for bad in (0, 1, 2, 5, 32, 128):
        assert _set_fanout(ctx, bad) == TC_ERR_ARG
    assert ctx.lib.tc_dbg_fm_set_lcp_fanout(None, 64) == TC_ERR_ARG
    for f in (4, 8, 16, 64):                        # part 3 follows the fan-out, the answers do not
        assert _set_fanout(ctx, f) == 0
        tb = _text(0x6680, 700, b"ACGT")
        fm = ctx.fm_build(tb, lcp=True)
        try:
            assert fm.device_bytes(3) == 4 * (701 + _tree_words(701, f))
            pats = _patterns(0x6681, tb, b"ACGT")
            assert _same(fm.match_stats(pats), R.Ref(tb).match_stats(pats))
        finally:
            fm.close()
    assert _set_fanout(ctx, 64) == 0


# ------------------------------------------------------------------------------------------------ 3: one divergent batch
def test_divergent_batch(ctx):
    """600 patterns of lengths 0 .. 300 in one launch: more than one workgroup, lanes finishing far apart"""
    tb = _text(0x6700, 4161, b"ACGNT")
    rng = np.random.default_rng(0x6701)
    al = np.frombuffer(b"ACGNT", np.uint8)
    lens = [0, 300] + [int(v) for v in rng.integers(0, 301, 598)]
    pats = []
    for i, m in enumerate(lens):
        if i % 3 == 0 and m:                # a mosaic of substrings: long matches, then shrinks
            p = b""
            while len(p) < m:
                p += _sub(rng, tb, int(rng.integers(1, 60)))
            pats.append(p[:m])
        else:                               # random: matches of about log_5 n bytes
            pats.append(al[rng.integers(0, 5, m)].tobytes())
    _every_way(ctx, tb, pats, min_lens=(8,))


# ------------------------------------------------------------------------------------------------ 4: the MEM protocol
def _raw_mems(fm, pats, min_len, cap, arrays):
    from textcomp import FMIndexHandle
    ctx = fm._ctx
    moffs = np.full(len(pats) + 1, 99, np.uint64)
    nm = C.c_uint64(cap)
    flat, offs = FMIndexHandle._pack(pats)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.tc_fm_mems(ctx.handle, fm._h, p(flat), p(offs), len(pats), min_len, p(moffs), p(arrays[0]), p(arrays[1]),
                            p(arrays[2]), C.byref(nm))
    return rc, int(nm.value), moffs


@pytest.mark.parametrize("sa_rate", [1, 4])
def test_mem_protocol(ctx, sa_rate):
    import torch
    tb = _text(0x6800, 700, b"ACGT")
    m = 40
    rng = np.random.default_rng(0x6801)
    pats = [p[:m] for p in _patterns(0x6802, tb, b"ACGT") if len(p) >= m] + [_sub(rng, tb, m), _sub(rng, tb, 25) + _sub(rng, tb, 15)]
    assert len(pats) >= 6 and all(len(p) == m for p in pats)
    ms = R.Ref(tb).match_stats(pats)
    fm = ctx.fm_build(tb, sa_rate=sa_rate, lcp=True)
    try:
        for min_len in (1, 2, 20, m, m + 1):
            want = R.mems(pats, ms, min_len)
            total = len(want[1])
            assert (total == 0) == (min_len == m + 1) and want[0][-1] == total
            assert _same(fm.mems(pats, min_len), want) and _same(_mems_dev(fm, pats, min_len), want)
            fresh = lambda: (np.full(total + 1, 0x77, np.uint64), np.full(total + 1, 0x77, np.uint64), np.full(total + 1, 0x77, np.uint32))
            # sizes only
            rc, nm, moffs = _raw_mems(fm, pats, min_len, 0, (None, None, None))
            assert rc == 0 and nm == total and np.array_equal(moffs, want[0])
            if total == 0:
                continue
            # one short: the total, the payload untouched
            arr = fresh()
            rc, nm, _ = _raw_mems(fm, pats, min_len, total - 1, arr)
            assert rc == TC_ERR_CAPACITY and nm == total and all((a == 0x77).all() for a in arr)
            # exactly enough
            rc, nm, moffs = _raw_mems(fm, pats, min_len, total, arr)
            assert rc == 0 and nm == total and _same((moffs, arr[0][:total], arr[1][:total], arr[2][:total]), want)
            assert all(a[total] == 0x77 for a in arr)
            # one of the arrays missing, or none with a capacity: an argument error
            assert _raw_mems(fm, pats, min_len, total, (arr[0], None, arr[2]))[0] == TC_ERR_ARG
            assert _raw_mems(fm, pats, min_len, total, (None, None, None))[0] == TC_ERR_ARG
            # the same on the device
            d_flat, d_offs, _ = _dev_patterns(pats)
            d_moffs = torch.zeros(len(pats) + 1, dtype=torch.int64, device="cuda")
            d_arr = [torch.full((total,), 0x77, dtype=dt, device="cuda") for dt in (torch.int64, torch.int64, torch.int32)]
            torch.cuda.synchronize()

            def call(cap):
                nm = C.c_uint64(cap)
                rc = ctx.lib.tc_fm_mems_dev(ctx.handle, fm._h, C.c_void_p(d_flat.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                            len(pats), min_len, C.c_void_p(d_moffs.data_ptr()), C.c_void_p(d_arr[0].data_ptr()),
                                            C.c_void_p(d_arr[1].data_ptr()), C.c_void_p(d_arr[2].data_ptr()), C.byref(nm))
                return rc, int(nm.value)

            assert call(total - 1) == (TC_ERR_CAPACITY, total)
            assert all(bool((a == 0x77).all()) for a in d_arr)
            assert call(total) == (0, total)
            assert _same((_np(d_moffs, np.uint64), _np(d_arr[0], np.uint64), _np(d_arr[1], np.uint64), _np(d_arr[2], np.uint32)), want)
        # min_len = 0
        arr = (np.zeros(8, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint32))
        assert _raw_mems(fm, pats, 0, 8, arr)[0] == TC_ERR_ARG
        assert _raw_mems(fm, pats, 0, 0, (None, None, None))[0] == TC_ERR_ARG
    finally:
        fm.close()


# ------------------------------------------------------------------------------------------------ 5: edges and errors
def _raw_ms(ctx, h, flat, offs, npat, ms_len, ms_pos, ms_occ):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.lib.tc_fm_match_stats(ctx.handle, h, p(flat), p(offs), npat, p(ms_len), p(ms_pos), p(ms_occ))


def test_edges_and_errors(ctx):
    import textcomp
    from textcomp import FMIndexHandle
    tb = _text(0x6900, 600, b"ACGT")
    pats = _patterns(0x6901, tb, b"ACGT")
    want = R.Ref(tb).match_stats(pats)
    flat, offs = FMIndexHandle._pack(pats)
    total = int(offs[-1])
    fm = ctx.fm_build(tb, sa_rate=4, text_rate=4, lcp=True)
    plain = ctx.fm_build(tb, sa_rate=4, text_rate=4)
    empty = ctx.fm_build(b"", lcp=True)
    try:
        # NULL ms_pos / ms_occ in every combination; the arrays that are given are the reference's
        for with_pos in (False, True):
            for with_occ in (False, True):
                got = fm.match_stats(pats, pos=with_pos, occ=with_occ)
                assert np.array_equal(got[0], want[0])
                assert (got[1] is None) if not with_pos else np.array_equal(got[1], want[1])
                assert (got[2] is None) if not with_occ else np.array_equal(got[2], want[2])
                d_flat, d_offs, _ = _dev_patterns(pats)
                got = fm.match_stats_dev(d_flat, d_offs, len(pats), total, pos=with_pos, occ=with_occ)
                assert np.array_equal(_np(got[0], np.uint32), want[0])
                assert (got[1] is None) if not with_pos else np.array_equal(_np(got[1], np.uint64), want[1])
                assert (got[2] is None) if not with_occ else np.array_equal(_np(got[2], np.uint32), want[2])
        # null arguments
        l, p, o = np.zeros(total, np.uint32), np.zeros(total, np.uint64), np.zeros(total, np.uint32)
        assert _raw_ms(ctx, None, flat, offs, len(pats), l, p, o) == TC_ERR_ARG
        assert _raw_ms(ctx, fm._h, None, offs, len(pats), l, p, o) == TC_ERR_ARG
        assert _raw_ms(ctx, fm._h, flat, None, len(pats), l, p, o) == TC_ERR_ARG
        assert _raw_ms(ctx, fm._h, flat, offs, len(pats), None, p, o) == TC_ERR_ARG
        nm = C.c_uint64(0)
        assert ctx.lib.tc_fm_mems(ctx.handle, None, None, None, 0, 1, None, None, None, None, C.byref(nm)) == TC_ERR_ARG
        assert ctx.lib.tc_fm_mems(ctx.handle, fm._h, None, None, 3, 1, None, None, None, None, C.byref(nm)) == TC_ERR_ARG
        assert ctx.lib.tc_fm_mems(ctx.handle, fm._h, None, None, 3, 1, None, None, None, None, None) == TC_ERR_ARG
        # npat = 0
        assert _raw_ms(ctx, fm._h, None, None, 0, None, None, None) == 0
        nm = C.c_uint64(5)
        assert ctx.lib.tc_fm_mems(ctx.handle, fm._h, None, None, 0, 1, None, None, None, None, C.byref(nm)) == 0 and nm.value == 0
        assert _same(fm.mems([]), (np.zeros(1, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32)))
        # the empty index: all zeros and no MEMs, host and device
        assert empty.has_lcp is False and empty.device_bytes(3) == 0
        some = [b"AC", b"", b"\x00\xff"]
        z = (np.zeros(4, np.uint32), np.zeros(4, np.uint64), np.zeros(4, np.uint32))
        got = [np.full(4, 5, np.uint32), np.full(4, 5, np.uint64), np.full(4, 5, np.uint32)]
        f2, o2 = FMIndexHandle._pack(some)
        assert _raw_ms(ctx, empty._h, f2, o2, 3, *got) == 0 and _same(got, z)
        assert _same(_match_stats_dev(empty, some), z)
        assert _same(empty.mems(some), (np.zeros(4, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32)))
        assert _same(_mems_dev(empty, some, 1), (np.zeros(4, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint64), np.empty(0, np.uint32)))
        # an index without the LCP part, and an imported one (an import never has the part)
        back = textcomp.FMIndexHandle.import_dev(ctx, fm.export_dev(with_locate=True), n=len(tb))
        try:
            for other in (plain, back):
                assert other.has_lcp is False
                with pytest.raises(textcomp.TcError) as ei:
                    other.match_stats(pats)
                assert ei.value.code == TC_ERR_ARG
                with pytest.raises(textcomp.TcError) as ei:
                    other.mems(pats)
                assert ei.value.code == TC_ERR_ARG
                with pytest.raises(textcomp.TcError) as ei:
                    _match_stats_dev(other, pats)
                assert ei.value.code == TC_ERR_ARG
        finally:
            back.close()
        # the build's arguments
        for sa_rate, text_rate in ((0, 0), (3, 0), (8192, 0), (4, 3), (4, 8192)):
            h = C.c_void_p(1)
            t8 = np.frombuffer(tb, np.uint8)
            rc = ctx.lib.tc_fm_build_lcp(ctx.handle, t8.ctypes.data_as(C.c_void_p), len(tb), sa_rate, text_rate, C.byref(h))
            assert rc == TC_ERR_ARG and not h.value
        # two contexts querying one index: scratch comes from the calling context
        other_ctx = textcomp.Context(0)
        try:
            borrowed = textcomp.FMIndexHandle(other_ctx, None, _handle=fm._h, _n=len(tb))
            try:
                for _ in range(2):
                    assert _same(borrowed.match_stats(pats), want) and _same(fm.match_stats(pats), want)
                    assert _same(borrowed.mems(pats, 2), R.mems(pats, want, 2)) and _same(fm.mems(pats, 2), R.mems(pats, want, 2))
            finally:
                borrowed._h = None          # the index stays the first context's
        finally:
            other_ctx.close()
    finally:
        fm.close()
        plain.close()
        empty.close()


# ------------------------------------------------------------------------------------------------ 6: nothing else moved
def _tree_words(N, f):
    """the words of the min tree over N rows: levels of ceil(previous / f) entries up to the first of at most f, every level
    rounded up to a multiple of 4 words (include/textcomp.h)"""
    words, cur = 0, N
    while True:
        cur = -(-cur // f)
        words += (cur + 3) // 4 * 4
        if cur <= f:
            return words


def _export_into_zeros(fm, with_locate):
    """tc_fm_export_dev into a zeroed buffer (the call leaves the alignment gaps between the parts as it finds them)"""
    import torch
    ctx = fm._ctx
    nb = int(ctx.lib.tc_fm_export_bound(fm._h, int(with_locate)))
    buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    used = C.c_uint64(nb)
    ctx._check(ctx.lib.tc_fm_export_dev(ctx.handle, fm._h, int(with_locate), C.c_void_p(buf.data_ptr()), C.byref(used)))
    return buf[:used.value]


@pytest.mark.parametrize("sa_rate,text_rate", [(1, 0), (4, 4)])
def test_nothing_else_moved(ctx, sa_rate, text_rate):
    """on an LCP-built index every other call answers what the same index without the part answers"""
    n = 4161
    tb = _text(0x6A00, n, b"ACGT")
    pats = _patterns(0x6A01, tb, b"ACGT")
    with_part = ctx.fm_build(tb, sa_rate=sa_rate, text_rate=text_rate, lcp=True)
    without = ctx.fm_build(tb, sa_rate=sa_rate, text_rate=text_rate)
    try:
        assert with_part.has_lcp is True and without.has_lcp is False
        assert (with_part.sa_rate, with_part.text_rate) == (without.sa_rate, without.text_rate) == (sa_rate, text_rate)
        assert np.array_equal(with_part.count(pats), without.count(pats))
        for a, b in zip(with_part.locate(pats), without.locate(pats)):
            assert np.array_equal(a, b)
        assert _same(with_part.factorize(pats), without.factorize(pats))
        short = [p for p in pats if len(p) <= 40]
        assert np.array_equal(with_part.count_mm(short, 1), without.count_mm(short, 1))
        if text_rate:
            starts, lens = [1, 7, n - 99, n + 1], [100, 0, 100, 0]
            assert with_part.extract(starts, lens) == without.extract(starts, lens) == [tb[s - 1:s - 1 + l] for s, l in zip(starts, lens)]
        part3 = 4 * (n + 1) + 4 * _tree_words(n + 1, 64)
        assert with_part.device_bytes(3) == part3 and without.device_bytes(3) == 0
        assert with_part.device_bytes(0) - part3 == without.device_bytes(0)
        assert with_part.device_bytes(1) == without.device_bytes(1) and with_part.device_bytes(2) == without.device_bytes(2)
        assert with_part.device_bytes(4) == 0
        for with_locate in (False, True):
            a, b = _export_into_zeros(with_part, with_locate), _export_into_zeros(without, with_locate)
            assert a.numel() == b.numel() and bool((a == b).all())
    finally:
        with_part.close()
        without.close()


# ------------------------------------------------------------------------------------------------ 7: against factorize
def test_cross_check_against_factorize(ctx):
    """the rightmost factor of a pattern, of length l, is the matching statistic at m - l, and the one before it does
    not reach past it"""
    tb = _text(0x6B00, 2000, b"ACGNT")
    pats = [p for p in _patterns(0x6B01, tb, b"ACGNT") if p]
    fm = ctx.fm_build(tb, lcp=True)
    try:
        foffs, fpos, flen = fm.factorize(pats)
        assert _same((foffs, fpos, flen), factor_ref.factorize(tb, pats))
        ms_len, ms_pos, _ = fm.match_stats(pats)
        o = 0
        for j, p in enumerate(pats):
            m, last = len(p), int(foffs[j + 1]) - 1
            l = int(flen[last])
            if l == 0:                      # a literal: the byte does not occur
                assert ms_len[o + m - 1] == 0
            else:
                assert ms_len[o + m - l] == l and ms_pos[o + m - l] == fpos[last]
                if m > l:
                    assert ms_len[o + m - l - 1] <= l
            o += m
    finally:
        fm.close()


def test_fmindex_mirrors(ctx):
    from textcomp import fmindex
    res = fmindex.bytestringFMIndexMatchStatsS([b"ACGX", b""], b"TTACGTT", ctx)
    assert res == [(b"ACGX", [(3, 3, 1), (2, 4, 1), (1, 5, 1), (0, 0, 0)]), (b"", [])]
    assert fmindex.textFMIndexMatchStatsP(["ACGX"], "TTACGTT", ctx) == [("ACGX", res[0][1])]
    assert fmindex.bytestringFMIndexMemsS([b"ACGX", b""], b"TTACGTT", 1, ctx) == [(b"ACGX", [(0, 3, 3)]), (b"", [])]
    assert fmindex.textFMIndexMemsP(["ACGX"], "TTACGTT", 2, ctx) == [("ACGX", [(0, 3, 3)])]
    assert fmindex.bytestringFMIndexMemsP([], b"TTACGTT", 1, ctx) == []
