"""FM-index extract (tc_fm_build_self, tc_fm_extract, tc_fm_extract_dev): text ranges read back from the index.

"Equal" always means: equal to the Python slice tb[start - 1 : start - 1 + len] -- start is 1-based, exactly as
tc_fm_locate answers positions.  That slice is the whole oracle.

The malformed-import cases check error RETURNS that the walk's bounds guarantee (csrc/tc_fm_host.hpp,
fm_extract_walk_kernel: the step count is fixed by the query, every row < N, the sample index within the samples, no
step from the primary row or from a byte without a code); they are not there to shake the device."""
import ctypes as C
import threading
import traceback

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw_host(ctx, fm, starts, lens, cap=None, pad=24):
    """tc_fm_extract on numpy arrays with a canary-filled out -> (rc, nbytes, offs, out-with-canaries, pad)"""
    st = np.asarray(starts, np.uint64); ln = np.asarray(lens, np.uint64)
    total = int(sum(int(v) for v in lens)) if cap is None else cap
    buf = np.full(total + 2 * pad, CANARY, np.uint8)
    offs = np.zeros(len(st) + 1, np.uint64)
    nb = C.c_uint64(total)
    rc = ctx.lib.tc_fm_extract(ctx.handle, fm._h, _p(st), _p(ln), len(st), _p(offs), C.c_void_p(buf.ctypes.data + pad), C.byref(nb))
    return rc, int(nb.value), offs, buf


def _raw_dev(ctx, fm, starts, lens, cap=None, pad=24, shift=0):
    """tc_fm_extract_dev likewise; `shift` moves d_out off its 8-byte alignment"""
    import torch
    st = torch.from_numpy(np.asarray(starts, np.uint64).view(np.int64).copy()).cuda()
    ln = torch.from_numpy(np.asarray(lens, np.uint64).view(np.int64).copy()).cuda()
    total = int(sum(int(v) for v in lens)) if cap is None else cap
    buf = torch.full((total + 2 * pad + 8,), CANARY, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(len(starts) + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nb = C.c_uint64(total)
    rc = ctx.lib.tc_fm_extract_dev(ctx.handle, fm._h, C.c_void_p(st.data_ptr()), C.c_void_p(ln.data_ptr()), len(starts),
                                   C.c_void_p(offs.data_ptr()), C.c_void_p(buf.data_ptr() + pad + shift), C.byref(nb))
    return rc, int(nb.value), offs.cpu().numpy().astype(np.uint64), buf.cpu().numpy()[shift:]


def _check_queries(ctx, fm, tb, queries, shift=0, what=""):
    """both entry points, canaries around out: every query equals the slice and nothing else is written"""
    starts = [s for s, _ in queries]; lens = [l for _, l in queries]
    want = b"".join(tb[s - 1:s - 1 + l] for s, l in queries)
    want_offs = np.cumsum([0] + lens).astype(np.uint64)
    pad = 24
    for raw in (_raw_host(ctx, fm, starts, lens, pad=pad), _raw_dev(ctx, fm, starts, lens, pad=pad, shift=shift)):
        rc, nb, offs, buf = raw
        assert rc == 0, (what, rc, ctx.lib.tc_last_error(ctx.handle))
        assert nb == len(want), what
        assert np.array_equal(offs, want_offs), what
        got = buf[pad:pad + nb].tobytes()
        if got != want:
            bad = next(i for i in range(len(queries)) if got[int(offs[i]):int(offs[i + 1])] != tb[starts[i] - 1:starts[i] - 1 + lens[i]])
            raise AssertionError("%s: query %d = %r differs" % (what, bad, queries[bad]))
        assert (buf[:pad] == CANARY).all() and (buf[pad + nb:pad + nb + pad] == CANARY).all(), what + ": canary overwritten"


def _all_pairs(n):
    return [(s, l) for s in range(1, n + 2) for l in range(0, n - s + 2)]


# ------------------------------------------------------------------------------------------------ 1
def test_doc_and_small_texts(ctx, golden):
    doc = golden["fmindex_doc"]["text"].encode()
    src = golden["source"].encode()
    texts = [doc, src, b"a", b"ab", b"aaaa", b"mississippi", bytes(range(256))]
    for tb in texts:
        n = len(tb)
        queries = _all_pairs(n) if n <= 16 else _all_pairs(n)[::7] + [(1, n), (n, 1), (1, 1), (n + 1, 0)]
        for tr in (1, 2, 4, 32, 4096):
            for sr in (1, 8):
                fm = ctx.fm_build(tb, sa_rate=sr, text_rate=tr)
                assert fm.text_rate == tr and fm.sa_rate == sr
                assert fm.device_bytes(2) == 4 * (n // tr + 1)
                assert fm.extract([1], [n]) == [tb]                      # the whole text as one query
                _check_queries(ctx, fm, tb, queries, what="n %d rates %d/%d" % (n, sr, tr))
                if tr in (2, 32):
                    assert fm.extract([s for s, _ in queries], [l for _, l in queries]) == [tb[s - 1:s - 1 + l] for s, l in queries]
                # extract(hit, |pattern|) returns the pattern
                pats = [p for p in (tb[:1], tb[-1:], tb[1:4], tb[n // 2:n // 2 + 3], tb) if p]
                hits = fm.locate(pats)
                for p, h in zip(pats, hits):
                    assert len(h) >= 1
                    assert fm.extract(h, [len(p)] * len(h)) == [p] * len(h)
                fm.close()


# ------------------------------------------------------------------------------------------------ 2
def _boundary_queries(n, r):
    qs = [(1, 0), (n + 1, 0), (1, 1), (1, n), (n, 1), (1, min(n, 3 * r + 5)), (max(1, n - 3 * r - 4), min(n, 3 * r + 5))]
    # starts and ends on multiples of r and one to either side (0-based a, e)
    for m in range(0, n + r, r):
        for a in (m - 1, m, m + 1):
            for e in (a, a + 1, a + r - 1, a + r, a + r + 1, a + 2 * r + 1, m + r - 1, m + r, m + r + 1):
                if 0 <= a <= e <= n:
                    qs.append((a + 1, e - a))
        if len(qs) > 1200:
            break
    for e in (n,):                                   # the anchor is row 0
        for a in (e - 1, e - r, e - r - 1, e - 2 * r - 3, 0):
            if 0 <= a <= e:
                qs.append((a + 1, e - a))
    # inside one segment; over at least 3 segments
    if n > r + 6:
        qs.append((r + 3, min(3, r - 2)))
    if n >= 3 * r + 2:
        qs.append((r // 2 + 1, 2 * r + r // 2 + 1))
    return qs


@pytest.mark.parametrize("r", [16, 64, 4096])
def test_boundaries(ctx, r):
    rng = np.random.default_rng(0xE7 + r)
    for n in (447, 448, 449, 895, 896, 4095, 4096, 4097):
        tb = rng.integers(97, 101, n).astype(np.uint8).tobytes()
        fm = ctx.fm_build(tb, sa_rate=8 if n % 2 else 1, text_rate=r)
        assert fm.text_rate == r and fm.device_bytes(2) == 4 * (n // r + 1)
        _check_queries(ctx, fm, tb, _boundary_queries(n, r), what="n %d r %d" % (n, r))
        # lengths 1 .. 9 and 64 mixed in one call so that the pieces start at all 8 output alignments, twice over (a second
        # round after a length-1 piece), and the device buffer itself at every alignment
        lens = [1, 2, 3, 4, 5, 6, 7, 8, 9, 64] * 8 + [1] + [8, 64, 7, 9, 1, 2, 3, 4, 5, 6] * 4
        offs = np.cumsum([0] + lens)
        assert {int(o) % 8 for o, l in zip(offs, lens) if l in (8, 9, 64)} == set(range(8))
        starts = [int(v) for v in rng.integers(1, n - 64, len(lens))]
        starts[3] = 1; starts[9] = n - 63; starts[12] = r if r < n - 64 else 2
        for shift in range(8):
            _check_queries(ctx, fm, tb, list(zip(starts, lens)), shift=shift, what="mix n %d r %d shift %d" % (n, r, shift))
        fm.close()


# ------------------------------------------------------------------------------------------------ 3
def test_byte_zero_in_the_text(ctx):
    rng = np.random.default_rng(0xE73)
    mid = rng.integers(0, 3, 700).astype(np.uint8).tobytes()
    texts = [b"\0", b"\0" * 5, b"\0" * 1000, b"\0\0\0" + b"abc" * 50, b"abc" * 50 + b"\0\0\0", b"\0" + mid + b"\0", b"\0a\0b" * 120]
    for tb in texts:
        n = len(tb)
        for tr in (1, 4, 64, 4096):
            fm = ctx.fm_build(tb, sa_rate=1 if tr != 4 else 4, text_rate=tr)
            qs = [(1, n), (1, 1), (n, 1), (1, 0), (n + 1, 0)] + [(s, min(l, n - s + 1)) for s in range(1, n + 1, max(1, n // 37)) for l in (1, 2, 9, 70)]
            _check_queries(ctx, fm, tb, qs, what="zeros n %d r %d" % (n, tr))
            fm.close()


# ------------------------------------------------------------------------------------------------ 4
def test_randomized(ctx):
    rng = np.random.default_rng(0xE74)
    for it in range(30):
        n = int(rng.integers(1, 20001)) if it % 4 else int(rng.choice([1, 2, 63, 64, 65, 449, 4097, 20000]))
        if it == 0:
            t = np.full(n, 65, np.uint8)                                  # unary
        elif it == 1:
            t = np.frombuffer((b"abc" * n)[:n], np.uint8).copy()           # period 3
        else:
            sigma = (1, 2, 4, 5, 16, 200, 256)[it % 7]
            alpha = rng.permutation(256)[:sigma]
            t = alpha[rng.integers(0, sigma, n)].astype(np.uint8)
            if n > 8:
                ln = int(rng.integers(1, n // 2)); a0, b0 = int(rng.integers(0, n - ln)), int(rng.integers(0, n - ln))
                t[b0:b0 + ln] = t[a0:a0 + ln].copy()
        tb = t.tobytes()
        tr = int(2 ** rng.integers(0, 13)); sr = int(2 ** rng.integers(0, 7))
        fm = ctx.fm_build(tb, sa_rate=sr, text_rate=tr)
        qs = []
        for _ in range(200):
            a = int(rng.integers(0, n + 1))
            mx = n - a
            l = int(rng.integers(0, mx + 1)) if rng.integers(0, 4) == 0 else int(min(mx, rng.integers(0, 130)))
            qs.append((a + 1, l))
        _check_queries(ctx, fm, tb, qs, shift=it % 8, what="it %d n %d rates %d/%d" % (it, n, sr, tr))
        fm.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("r", [32, 1024])
def test_whole_text_2_20(ctx, r):
    import torch
    n = 1 << 20
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx._check(ctx.lib.tc_generate_dev(ctx.handle, 0, 0xE75, n, C.c_void_p(d_text.data_ptr())))
    fm = ctx.fm_build_dev(d_text, sa_rate=32, text_rate=r)
    assert fm.text_rate == r and fm.device_bytes(2) == 4 * (n // r + 1)
    st = torch.tensor([1], dtype=torch.int64, device="cuda"); ln = torch.tensor([n], dtype=torch.int64, device="cuda")
    offs, out = fm.extract_dev(st, ln, 1, cap=n)
    assert offs.tolist() == [0, n] and out.numel() == n
    assert torch.equal(out, d_text)
    fm.close()


# ------------------------------------------------------------------------------------------------ 6
def test_errors(ctx):
    import torch
    from textcomp import TcError, _lib
    tb = O.gen_acgtn(0xE76, 5000).tobytes()
    n = len(tb)
    fm = ctx.fm_build(tb, sa_rate=8, text_rate=16)
    good = [(5, 100), (1, 7), (n - 9, 10)]
    for bad in ((0, 5), (n - 3, 5), (2, 2 ** 64 - 1), (n + 2, 0), (2 ** 64 - 1, 2), (0, 0)):
        qs = good[:2] + [bad] + good[2:]
        starts = [s for s, _ in qs]; lens = [l for _, l in qs]
        for raw in (_raw_host, _raw_dev):
            rc, nb, offs, buf = raw(ctx, fm, starts, lens, cap=4096)
            assert rc == _lib.TC_ERR_ARG, (bad, rc)
            assert (buf == CANARY).all(), "out was written to although a query was bad"
    # exactly at the end is fine
    _check_queries(ctx, fm, tb, [(n - 3, 4), (n + 1, 0), (1, n)])
    # capacity one byte short
    starts = [s for s, _ in good]; lens = [l for _, l in good]
    total = sum(lens)
    for raw in (_raw_host, _raw_dev):
        rc, nb, offs, buf = raw(ctx, fm, starts, lens, cap=total - 1)
        assert rc == _lib.TC_ERR_CAPACITY and nb == total
        assert (buf == CANARY).all(), "out was written to although the capacity did not suffice"
    # nq = 0
    nb = C.c_uint64(0)
    assert ctx.lib.tc_fm_extract(ctx.handle, fm._h, None, None, 0, None, None, C.byref(nb)) == 0 and nb.value == 0
    assert ctx.lib.tc_fm_extract_dev(ctx.handle, fm._h, None, None, 0, None, None, C.byref(nb)) == 0 and nb.value == 0
    assert fm.extract([], []) == []
    fm.close()
    # indexes without text samples
    for other in (ctx.fm_build(tb), ctx.fm_build(tb, sa_rate=8), ctx.fm_build(b"", sa_rate=2, text_rate=4)):
        assert other.text_rate == 0 and other.device_bytes(2) == 0
        assert int(ctx.lib.tc_fm_text_rate(other._h)) == 0
        for raw in (_raw_host, _raw_dev):
            rc, nb, offs, buf = raw(ctx, other, [1], [0], cap=16)
            assert rc == _lib.TC_ERR_ARG
            if other.n:
                assert b"tc_fm_build_self" in ctx.lib.tc_last_error(ctx.handle)
        with pytest.raises(TcError):
            other.extract([1], [0])
        other.close()
    # bad text rates (and bad sa rates beside a good text rate)
    t = np.frombuffer(b"abracadabra", np.uint8).copy()
    d_t = torch.from_numpy(t).cuda()
    torch.cuda.synchronize()
    for sr, tr in ((1, 0), (1, 3), (1, 8192), (8, 0), (8, 3), (8, 8192), (0, 4), (3, 4), (8192, 4)):
        for fn, ptr in ((ctx.lib.tc_fm_build_self, _p(t)), (ctx.lib.tc_fm_build_self_dev, C.c_void_p(d_t.data_ptr()))):
            h = C.c_void_p(0xDEAD)
            assert fn(ctx.handle, ptr, len(t), sr, tr, C.byref(h)) == _lib.TC_ERR_ARG, (sr, tr)
            assert not h.value, "*out must be null after a refused build"
    # the ctx still works
    fm = ctx.fm_build(bytes(t), sa_rate=1, text_rate=4096)
    assert fm.extract([1, 8], [4, 4]) == [b"abra", b"abra"] and sorted(fm.locate([b"abra"])[0].tolist()) == [1, 8]
    fm.close()
    assert ctx.encode(bytes(t))["n"] == len(t)


# ------------------------------------------------------------------------------------------------ 7
# the export's layout (csrc/tc_fm_host.hpp, FmWire): a 1600-byte header padded to 256, then every part padded to 256
_HDR = 1792
_OFF_N, _OFF_PRIMARY, _OFF_LINES, _OFF_BYTES, _OFF_SIGMA, _OFF_WITH_LOCATE, _OFF_PAIRS, _OFF_RATE = 8, 24, 32, 40, 48, 52, 56, 60


def _al(v):
    return (v + 255) & ~255


def _u32_at(buf, off):
    return int(buf[off:off + 4].cpu().numpy().view(np.uint32)[0])


def _u64_at(buf, off):
    return int(buf[off:off + 8].cpu().numpy().view(np.uint64)[0])


def _put_u32(buf, off, v):
    import torch
    buf[off:off + 4] = torch.from_numpy(np.array([v], np.uint32).view(np.uint8).copy()).to(buf.device)


def test_export_import(ctx):
    import textcomp
    import torch
    from textcomp import FMIndexHandle, TcError, TcMalformed, _lib
    n, sr, tr = 20_000, 8, 16
    tb = O.gen_acgtn(0xE77, n).tobytes()
    N, lines, nisa, nsamp = n + 1, (n + 1) // 448 + 1, n // tr + 1, n // sr + 1
    rng = np.random.default_rng(0xE77)
    qs = [(1, n), (1, 1), (n, 1), (n + 1, 0)] + [(int(a) + 1, int(min(n - a, l))) for a, l in zip(rng.integers(0, n, 300), rng.integers(0, 200, 300))]
    starts = [s for s, _ in qs]; lens = [l for _, l in qs]
    want = [tb[s - 1:s - 1 + l] for s, l in qs]
    plain = ctx.fm_build(tb, sa_rate=sr)
    fm = ctx.fm_build(tb, sa_rate=sr, text_rate=tr)
    full_self = ctx.fm_build(tb, sa_rate=1, text_rate=tr)
    ctx2 = textcomp.Context(0)
    try:
        assert fm.extract(starts, lens) == want and full_self.extract(starts, lens) == want
        # device bytes: parts 0 and 1 of the indexes without text samples are the header's formulas, the self index adds part 2
        sig = 5
        count_part = 768 * 4 + sig * lines * 64 + sig * sig * lines * 64 + 25 * 4
        assert plain.device_bytes(1) == (N + 16) + lines * 64 + 4 * nsamp and plain.device_bytes(2) == 0
        assert plain.device_bytes(0) == plain.device_bytes(1) + count_part
        full = ctx.fm_build(tb)
        assert full.device_bytes(1) == (N + 16) + 4 * N and full.device_bytes(0) == full.device_bytes(1) + count_part and full.device_bytes(2) == 0
        full.close()
        assert fm.device_bytes(2) == 4 * nisa and fm.device_bytes(1) == plain.device_bytes(1)
        assert fm.device_bytes(0) == plain.device_bytes(0) + 4 * nisa
        assert fm.device_bytes(3) == 0 and fm.device_bytes(-1) == 0

        # the export: the sampled index's bytes up to the header word, then the samples
        bp = plain.export_dev(with_locate=True)
        b1 = fm.export_dev(with_locate=True)
        assert int(ctx.lib.tc_fm_export_bound(fm._h, 1)) == b1.numel() == bp.numel() + _al(4 * nisa)
        assert _u32_at(bp, _OFF_WITH_LOCATE) == 1 and _u32_at(b1, _OFF_WITH_LOCATE) == (1 | tr << 8)
        assert bp[:8].cpu().numpy().tobytes() == b"TCFMI02\0" == b1[:8].cpu().numpy().tobytes()
        assert _u64_at(b1, _OFF_BYTES) == b1.numel() and _u64_at(bp, _OFF_BYTES) == bp.numel()
        assert _u32_at(b1, _OFF_RATE) == sr == _u32_at(bp, _OFF_RATE)
        hp, h1 = bp[:1600].clone(), b1[:1600].clone()
        for off, size in ((_OFF_BYTES, 8), (_OFF_WITH_LOCATE, 4)):
            hp[off:off + size] = 0; h1[off:off + size] = 0
        assert torch.equal(hp, h1)
        o = _HDR
        for name, size in (("bits", sig * lines * 64), ("bits2", sig * sig * lines * 64), ("L", N), ("marks", lines * 64), ("samples", 4 * nsamp)):
            assert torch.equal(bp[o:o + size], b1[o:o + size]), name
            o += _al(size if name != "L" else N + 16)
        assert o == bp.numel()
        o_isa = o
        isa = b1[o_isa:o_isa + 4 * nisa].cpu().numpy().view(np.uint32)
        primary = _u64_at(b1, _OFF_PRIMARY)
        assert int(isa[0]) == primary and int(isa.max()) < N and len(set(isa.tolist())) == nisa
        # without the locate part nothing of it is shipped
        b0 = fm.export_dev(with_locate=False)
        assert b0.numel() == plain.export_dev(with_locate=False).numel() and _u32_at(b0, _OFF_WITH_LOCATE) == 0

        # round trips
        imp = FMIndexHandle.import_dev(ctx2, b1.clone(), n=n)
        assert imp.text_rate == tr and imp.sa_rate == sr and imp.device_bytes(2) == fm.device_bytes(2) and imp.device_bytes(0) == fm.device_bytes(0)
        assert imp.extract(starts, lens) == want
        _check_queries(ctx2, imp, tb, qs[:50])
        assert [h.tolist() for h in imp.locate([tb[100:112]])] == [h.tolist() for h in plain.locate([tb[100:112]])]
        imp.close()
        bfs = full_self.export_dev(with_locate=True)
        imp = FMIndexHandle.import_dev(ctx2, bfs, n=n)
        assert imp.text_rate == tr and imp.sa_rate == 1 and imp.extract(starts, lens) == want
        imp.close()
        imp0 = FMIndexHandle.import_dev(ctx2, b0, n=n)
        assert imp0.text_rate == 0 and imp0.device_bytes(2) == 0
        with pytest.raises(TcError) as ei:
            imp0.extract(starts, lens)
        assert ei.value.code == _lib.TC_ERR_ARG
        imp0.close()

        # malformed imports, by their return values
        def refused(mut):
            b = b1.clone(); mut(b)
            with pytest.raises(TcMalformed):
                FMIndexHandle.import_dev(ctx2, b, n=n)
        refused(lambda b: _put_u32(b, o_isa, (primary + 1) % N))                 # isa[0] != primary
        refused(lambda b: _put_u32(b, o_isa + 4 * (nisa // 2), N))               # a sample >= N
        refused(lambda b: _put_u32(b, o_isa + 4 * (nisa - 1), 0xFFFFFFFF))
        refused(lambda b: _put_u32(b, _OFF_WITH_LOCATE, 1 | 3 << 8))             # bad rates in the header word
        refused(lambda b: _put_u32(b, _OFF_WITH_LOCATE, 1 | 8192 << 8))
        refused(lambda b: _put_u32(b, _OFF_WITH_LOCATE, 1 | (2 * tr) << 8))      # a valid rate, but the size does not follow from it
        refused(lambda b: _put_u32(b, _OFF_WITH_LOCATE, 1))                      # samples shipped, none announced
        refused(lambda b: _put_u32(b, _OFF_WITH_LOCATE, tr << 8))                # samples without a locate part
        b = bp.clone(); _put_u32(b, _OFF_WITH_LOCATE, 1 | tr << 8)              # an export without samples relabelled
        with pytest.raises(TcMalformed):
            FMIndexHandle.import_dev(ctx2, b, n=n)
        # an anchor that points at the primary row: the import cannot know, the walk that uses it stops
        kbad = 7
        b = b1.clone(); _put_u32(b, o_isa + 4 * kbad, primary)
        bad = FMIndexHandle.import_dev(ctx2, b, n=n)
        assert bad.text_rate == tr
        for call in (lambda: bad.extract([(kbad - 1) * tr + 3], [5]), lambda: _raw_dev(ctx2, bad, [(kbad - 1) * tr + 3], [5])[0]):
            try:
                rc = call()
            except TcMalformed:
                rc = _lib.TC_ERR_MALFORMED
            assert rc == _lib.TC_ERR_MALFORMED
        assert bad.extract([kbad * tr + 1], [tr]) == [tb[kbad * tr:(kbad + 1) * tr]]    # other anchors are fine
        bad.close()
        # later calls on good indexes succeed, on both contexts
        imp = FMIndexHandle.import_dev(ctx2, b1, n=n)
        assert imp.extract(starts, lens) == want
        imp.close()
        assert fm.extract(starts, lens) == want
    finally:
        ctx2.close()
        fm.close(); plain.close(); full_self.close()


# ------------------------------------------------------------------------------------------------ 8
def test_two_contexts_one_index():
    import textcomp
    from textcomp import FMIndexHandle
    n = 1 << 18
    tb = O.gen_acgtn(0xE78, n).tobytes()
    rng = np.random.default_rng(0xE78)
    owner = textcomp.Context(0)
    fm = owner.fm_build(tb, sa_rate=16, text_rate=32)
    ctxs = [textcomp.Context(0), textcomp.Context(0)]
    batches, wants = [], []
    for i in range(2):
        a = rng.integers(0, n - 300, 2000); l = rng.integers(0, 300, 2000)
        batches.append((a + 1, l))
        wants.append([tb[int(x):int(x) + int(y)] for x, y in zip(a, l)])
    errs, start = [], threading.Barrier(2)

    def work(i):
        try:
            import torch
            view = FMIndexHandle(ctxs[i], None, _handle=fm._h, _n=n)     # the owner's index, queried by this context
            try:
                d_st = torch.from_numpy(batches[i][0].astype(np.int64)).cuda()
                d_ln = torch.from_numpy(batches[i][1].astype(np.int64)).cuda()
                start.wait()
                for rep in range(20):
                    if rep % 2:
                        got = view.extract(batches[i][0], batches[i][1])
                    else:
                        offs, out = view.extract_dev(d_st, d_ln, 2000, cap=int(batches[i][1].sum()))
                        o, blob = offs.cpu().numpy(), out.cpu().numpy().tobytes()
                        got = [blob[int(o[q]):int(o[q + 1])] for q in range(2000)]
                    assert got == wants[i], (i, rep)
            finally:
                view._h = None                                            # not ours to free
        except Exception:
            errs.append(traceback.format_exc())

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    try:
        assert not errs, "\n".join(errs)
    finally:
        for c in ctxs: c.close()
        fm.close(); owner.close()
