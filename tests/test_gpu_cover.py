"""The repeat cover of a text (tc_repeat_spans, tc_repeat_mask, tc_repeat_dedup, their _dev forms and the three tc_cover_*_dev calls
over an array of lengths) against the reference of tests/cover_ref.py (a dictionary of the L-mers and a difference array;
tests/test_cover_ref.py holds it to brute force over all substrings).  Everything is compared exactly -- spans, the count, the mask
with a map and without, the dedup -- through the host and the _dev entries, on the smallest shapes at which the kernels can go
wrong: sizes on both sides of one and two tiles of the cover passes and of one and two workgroups of the row kernel, unary and
periodic texts, every byte once, min_len 1, n and n + 1, min_occ 2, 3, 5 and above every count, a fan-out-4 tree of five levels,
arrays of lengths no text produces (a reach carried over three tiles, spans that meet tile boundaries, entries of 0xffffffff), the
capacity / sizes-only / error protocol, and texts of 270 000 bytes against the library's own LPF array, unique prefixes, k-mers and
matching statistics."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cover_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "text-compression_amd", "csrc")
# positions per workgroup of the cover passes; rows per workgroup of cov_seed_kernel
T = int(re.search(r"#define COV_TILE (\d+)", open(os.path.join(_CSRC, "tc_cov.hpp")).read()).group(1))
ROW_TILE = int(re.search(r"#define FM_MS_NT (\d+)\n#define FM_MS_KERNEL __global__", open(os.path.join(_CSRC, "tc_fm_ms.hpp")).read()).group(1))
TILE_SIZES = sorted({n for t in (T, ROW_TILE) for n in (t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1)})
KINDS = (R.ALL, R.LATER)
LOWER = np.arange(256, dtype=np.uint8)
LOWER[65:91] += 32


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
def _text(seed, n, sigma):
    rng = np.random.default_rng(seed)
    alpha = (np.arange(sigma) * 256 // sigma).astype(np.uint8) if sigma > 4 else np.frombuffer(b"ACGT", np.uint8)[:sigma]
    return alpha[rng.integers(0, sigma, n)].tobytes()


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _np(x):
    import torch
    if isinstance(x, torch.Tensor):
        a = x.cpu().numpy()
        return a.astype(np.uint32) if x.dtype == torch.int32 else a
    return x


def _dev(a, dtype=np.uint8):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(a, dtype) if isinstance(a, (bytes, bytearray)) else a).copy()).cuda()


def _same_spans(got, want, what):
    s, l, c = (_np(x) for x in got)
    ws, wl, wc = want
    assert s.dtype == np.uint32 and l.dtype == np.uint32, what
    assert (s.tolist(), l.tolist(), int(c)) == (ws.tolist(), wl.tolist(), wc), what


def _same_bytes(got, want, covered, what):
    out, c = got
    out = _np(out)
    want = np.frombuffer(want, np.uint8) if isinstance(want, bytes) else want
    assert out.dtype == np.uint8 and len(out) == len(want) and int(c) == covered, (what, len(out), len(want), int(c), covered)
    bad = np.nonzero(out != want)[0]
    assert len(bad) == 0, "%s: [%d] = %d, want %d" % (what, bad[0], out[bad[0]], want[bad[0]])


def _every_way(ctx, t, L, q, kind, what="", host=True):
    """spans, count, mask (with a map and without) and dedup through the host and the _dev entries; returns the spans"""
    t = bytes(t)
    cov = R.cover(t, L, q, kind)
    spans = R.spans(cov)
    covered = spans[2]
    tag = "%s n=%d L=%d q=%d kind=%d" % (what, len(t), L, q, kind)
    d_text = _dev(t)
    if host:
        assert ctx.repeat_cover_count(t, L, q, kind) == (len(spans[0]), covered), tag
        _same_spans(ctx.repeat_spans(t, L, q, kind), spans, tag + " spans host")
        _same_bytes(ctx.repeat_mask(t, L, q, kind, LOWER), R.mask(t, cov, LOWER), covered, tag + " mask host")
        _same_bytes(ctx.repeat_mask(t, L, q, kind), R.mask(t, cov), covered, tag + " 0/1 host")
        _same_bytes(ctx.repeat_dedup(t, L, q, kind), R.dedup(t, cov), covered, tag + " dedup host")
    assert ctx.repeat_cover_count_dev(d_text, L, q, kind) == (len(spans[0]), covered), tag
    _same_spans(ctx.repeat_spans_dev(d_text, L, q, kind), spans, tag + " spans dev")
    _same_bytes(ctx.repeat_mask_dev(d_text, L, q, kind, LOWER), R.mask(t, cov, LOWER), covered, tag + " mask dev")
    _same_bytes(ctx.repeat_mask_dev(d_text, L, q, kind), R.mask(t, cov), covered, tag + " 0/1 dev")
    _same_bytes(ctx.repeat_dedup_dev(d_text, L, q, kind), R.dedup(t, cov), covered, tag + " dedup dev")
    return list(zip(spans[0].tolist(), spans[1].tolist()))


def _general(ctx, ln, L, what=""):
    """the general form over an array of lengths, through spans, mask (map, no map, no text) and dedup"""
    ln = np.asarray(ln, np.uint32)
    n = len(ln)
    t = _text(0xC700 + n, n, 4)
    cov = R.cover_of_len(ln, L)
    spans = R.spans(cov)
    covered = spans[2]
    tag = "%s n=%d L=%d" % (what, n, L)
    import torch
    d_len, d_text = torch.from_numpy(ln.view(np.int32).copy()).cuda(), _dev(t)
    _same_spans(ctx.cover_spans_dev(d_len, L), spans, tag + " spans")
    _same_spans(ctx.cover_spans_dev(d_len, L, cap=n), spans, tag + " spans, capacity n")
    _same_bytes(ctx.cover_mask_dev(d_len, d_text, L, LOWER), R.mask(t, cov, LOWER), covered, tag + " mask")
    _same_bytes(ctx.cover_mask_dev(d_len, d_text, L), R.mask(t, cov), covered, tag + " 0/1")
    _same_bytes(ctx.cover_mask_dev(d_len, None, L), R.mask(t, cov), covered, tag + " 0/1 without a text")
    _same_bytes(ctx.cover_dedup_dev(d_len, d_text, L), R.dedup(t, cov), covered, tag + " dedup")
    _same_bytes(ctx.cover_dedup_dev(d_len, d_text, L, cap=n), R.dedup(t, cov), covered, tag + " dedup, capacity n")
    return list(zip(spans[0].tolist(), spans[1].tolist()))


# ------------------------------------------------------------------------------------------------ small texts
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"aa", b"ab"):
        for kind in KINDS:
            for L in (1, 2):
                _every_way(ctx, t, L, 2, kind, repr(t))
    assert _every_way(ctx, b"aa", 1, 2, R.ALL) == [(0, 2)] and _every_way(ctx, b"aa", 1, 2, R.LATER) == [(1, 1)]
    assert _every_way(ctx, b"ab", 1, 2, R.ALL) == []
    assert ctx.repeat_cover_count(b"", 1) == (0, 0) and ctx.repeat_dedup(b"", 1)[0].tobytes() == b""


def test_worked_examples(ctx):
    upper = np.arange(256, dtype=np.uint8)
    upper[97:123] -= 32
    table = [
        (b"mississippi", 2, 2, R.ALL, [(1, 7)], 7, b"mISSISSIppi", b"mppi"),
        (b"mississippi", 2, 2, R.LATER, [(4, 4)], 4, b"missISSIppi", b"missppi"),
        (b"mississippi", 1, 4, R.ALL, [(1, 7), (10, 1)], 8, b"mISSISSIppI", b"mpp"),
        (b"mississippi", 1, 4, R.LATER, [(3, 5), (10, 1)], 6, b"misSISSIppI", b"mispp"),
        (b"abcabcabc", 3, 3, R.ALL, [(0, 9)], 9, b"ABCABCABC", b""),
        (b"abcabcabc", 3, 2, R.LATER, [(3, 6)], 6, b"abcABCABC", b"abc"),
        (b"banana", 2, 2, R.LATER, [(3, 3)], 3, b"banANA", b"ban"),
        (b"aaaa", 2, 2, R.LATER, [(1, 3)], 3, b"aAAA", b"a"),
        (b"abcdabxcd", 2, 2, R.ALL, [(0, 6), (7, 2)], 8, b"ABCDABxCD", b"x"),
        (b"abcdabxcd", 2, 2, R.LATER, [(4, 2), (7, 2)], 4, b"abcdABxCD", b"abcdx"),
        (b"the cat sat; the cat ran", 4, 2, R.LATER, [(13, 8)], 8, b"the cat sat; THE CAT ran", b"the cat sat; ran"),
    ]
    for t, L, q, kind, spans, covered, msk, dd in table:
        assert _every_way(ctx, t, L, q, kind, repr(t)) == spans
        out, c = ctx.repeat_mask(t, L, q, kind, upper)
        assert (out.tobytes(), c) == (msk, covered)
        out, c = ctx.repeat_dedup_dev(_dev(t), L, q, kind)
        assert (_np(out).tobytes(), c) == (dd, covered)


@pytest.mark.parametrize("n", [2, 255, 256, 257, T + 1])
def test_unary_texts(ctx, n):
    t = b"a" * n
    for L in (1, 2, n - 1):
        for q in (2, 3):
            if n - L + 1 < q:
                continue
            assert _every_way(ctx, t, L, q, R.ALL, "unary") == [(0, n)]
            assert _every_way(ctx, t, L, q, R.LATER, "unary") == [(1, n - 1)]
    assert _every_way(ctx, t, n, 2, R.ALL, "unary, L = n") == []


def test_every_byte_once(ctx):
    t = bytes(range(256))
    for kind in KINDS:
        assert _every_way(ctx, t, 1, 2, kind, "every byte once") == []
    t = bytes(range(256)) + bytes(range(255, -1, -1))      # twice, no pair twice but the middle one
    assert _every_way(ctx, t, 1, 2, R.ALL, "every byte twice") == [(0, 512)]
    assert _every_way(ctx, t, 1, 2, R.LATER, "every byte twice") == [(256, 256)]
    assert _every_way(ctx, t, 2, 2, R.ALL, "every byte twice") == []


@pytest.mark.parametrize("p", [3, 7])
def test_periodic_texts(ctx, p):
    n = 1000
    t = (b"abcdefg"[:p] * (n // p + 1))[:n]
    for L, q in ((1, 2), (p, 2), (p + 1, 3), (20, 5), (n - p, 2), (n - p + 1, 2)):
        assert _every_way(ctx, t, L, q, R.ALL, "period %d" % p) == ([(0, n)] if L <= n - p * (q - 1) else [])
        assert _every_way(ctx, t, L, q, R.LATER, "period %d" % p) == ([(p, n - p)] if L <= n - p * (q - 1) else [])


@pytest.mark.parametrize("sigma", [2, 4, 96])
def test_random_texts(ctx, sigma):
    t = _text(0xC100 + sigma, 3000, sigma)
    most = max(np.bincount(np.frombuffer(t, np.uint8)).tolist())
    for kind in KINDS:
        for L, q in ((1, 2), (2, 3), (3, 5), (5, 2), (8, 3), (11, 2), (1, most), (1, most + 1)):
            spans = _every_way(ctx, t, L, q, kind, "random over %d" % sigma, host=(L, q) in ((2, 3), (5, 2)))
            if q == most + 1:
                assert spans == []          # min_occ above every count
    assert len(_every_way(ctx, t, 1, most, R.ALL)) > 0


@pytest.mark.parametrize("n", TILE_SIZES)
def test_tile_sizes(ctx, n):
    """n on both sides of one and two tiles of the cover passes and of one and two workgroups of rows"""
    t = _text(0xC200 + n, n, 4)
    for kind in KINDS:
        assert len(_every_way(ctx, t, 6, 2, kind, "tile sizes", host=False)) > 1
        _every_way(ctx, t, 5, 3, kind, "tile sizes", host=False)
    half = _text(0xC300 + n, n // 2, 4)
    t = half + b"N" * (n - 2 * len(half)) + half    # the second half is covered to the last byte: a span that ends at n
    assert _every_way(ctx, t, 20, 2, R.LATER, "text + copy")[-1] == (n - len(half), len(half))
    _every_way(ctx, t, 20, 2, R.ALL, "text + copy", host=False)


@pytest.mark.parametrize("n", [1, 2, 37, T + 3])
def test_min_len_edges(ctx, n):
    """min_len = 1, n and n + 1 (and far above)"""
    for t in (_text(0xC400 + n, n, 2), b"a" * n, (b"ab" * n)[:n]):
        for kind in KINDS:
            for L in (1, n, n + 1, 0xffffffff):
                spans = _every_way(ctx, t, L, 2, kind, "L edges")
                if L >= n:
                    assert spans == []      # one occurrence of the whole text; nothing longer


def test_fanout_4(ctx):
    """a min tree of five levels: both searches and the range minimum of cov_seed_kernel climb it"""
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        for t in (_text(0xC500, 1100, 2), _text(0xC501, 2200, 4), b"a" * 1100, (b"ab" * 1300), b"b" + b"a" * 2600,
                  _text(0xC502, 1100, 3) * 2):
            assert len(t) >= 1100
            for kind in KINDS:
                _every_way(ctx, t, 1, 3, kind, "fan-out 4", host=False)
                _every_way(ctx, t, 6, 3, kind, "fan-out 4", host=False)
                _every_way(ctx, t, 1, 2, kind, "fan-out 4", host=False)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0
    _every_way(ctx, _text(0xC500, 1100, 2), 6, 3, R.LATER, "fan-out 64 again")


# ------------------------------------------------------------------------------------------------ the general form
def test_general_all_zero(ctx):
    for n in (1, T, 3 * T + 1):
        assert _general(ctx, np.zeros(n, np.uint32), 1, "all zero") == []


def test_general_one_entry_carried_over_three_tiles(ctx):
    ln = np.zeros(5 * T, np.uint32)
    ln[0] = 3 * T + 5
    assert _general(ctx, ln, 1, "one entry") == [(0, 3 * T + 5)]
    assert _general(ctx, ln, 3 * T + 5, "one entry, L = its length") == [(0, 3 * T + 5)]
    assert _general(ctx, ln, 3 * T + 6, "one entry, L above it") == []
    ln = np.zeros(5 * T, np.uint32)
    ln[T - 3] = 3 * T                       # from inside one tile over three whole ones to the middle of the last
    assert _general(ctx, ln, 2, "one entry") == [(T - 3, 3 * T)]


def test_general_tile_boundaries(ctx):
    ln = np.zeros(3 * T, np.uint32)
    ln[5] = T - 5                           # a reach that ends exactly on a tile boundary
    ln[2 * T - 1] = 1                       # a span that starts on a tile's last position (and ends there)
    assert _general(ctx, ln, 1, "boundaries") == [(5, T - 5), (2 * T - 1, 1)]
    ln[2 * T - 1] = 4                       # ... and goes on into the next tile
    assert _general(ctx, ln, 1, "boundaries") == [(5, T - 5), (2 * T - 1, 4)]
    ln = np.zeros(3 * T, np.uint32)
    ln[T + 1] = T - 2                       # two spans one byte apart across a tile boundary: [T + 1, 2T - 1) and [2T, 2T + 3)
    ln[2 * T] = 3
    assert _general(ctx, ln, 1, "one byte apart") == [(T + 1, T - 2), (2 * T, 3)]
    ln[2 * T - 1] = 1                       # the byte between them: one span
    assert _general(ctx, ln, 1, "joined") == [(T + 1, T + 2)]
    ln = np.zeros(2 * T, np.uint32)
    ln[T - 1] = 1
    ln[T] = 1                               # two positions that touch across the boundary: one span
    assert _general(ctx, ln, 1, "touching") == [(T - 1, 2)]


def test_general_huge_entries(ctx):
    """entries of 0xffffffff: the sum in 64 bits, the clamp to n"""
    for n in (1, 9, T + 7):
        ln = np.zeros(n, np.uint32)
        ln[n // 2] = 0xffffffff
        assert _general(ctx, ln, 1, "0xffffffff") == [(n // 2, n - n // 2)]
        assert _general(ctx, ln, 0xffffffff, "0xffffffff, L too") == [(n // 2, n - n // 2)]
        assert _general(ctx, np.full(n, 0xffffffff, np.uint32), 7, "all 0xffffffff") == [(0, n)]
    ln = np.zeros(2 * T + 1, np.uint32)
    ln[2 * T] = 0xfffffffe                  # the last position alone
    assert _general(ctx, ln, 5, "the last position") == [(2 * T, 1)]


def test_general_every_entry_counts_or_none(ctx):
    for n in (1, T - 1, 2 * T + 1):
        assert _general(ctx, np.full(n, 3, np.uint32), 3, "every entry") == [(0, n)]
        assert _general(ctx, np.full(n, 3, np.uint32), 4, "min_len above every entry") == []
        assert _general(ctx, np.full(n, 1, np.uint32), 1, "every entry, length 1") == [(0, n)]


def test_general_random_arrays(ctx):
    rng = np.random.default_rng(0xC600)
    for n, dense in ((2 * T + 100, 0.01), (3 * T - 1, 0.3)):
        ln = np.where(rng.random(n) < dense, rng.integers(0, 40, n), 0).astype(np.uint32)
        for L in (1, 5, 39, 41):
            _general(ctx, ln, L, "random lengths")
    import torch
    d_len = torch.from_numpy(ln.view(np.int32).copy()).cuda()
    cov = R.cover_of_len(ln[1:], 5)
    covered = int(cov.sum())
    _same_spans(ctx.cover_spans_dev(d_len[1:], 5), R.spans(cov), "an array that is only 4-byte aligned")
    t = _text(1, n, 4)
    d_text = _dev(t)
    _same_bytes(ctx.cover_mask_dev(d_len[1:], d_text[1:], 5, LOWER), R.mask(t[1:], cov, LOWER), covered, "... and an unaligned text")
    _same_bytes(ctx.cover_dedup_dev(d_len[1:], d_text[1:], 5), R.dedup(t[1:], cov), covered, "an unaligned text, dedup")


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ref(x):
    return C.byref(x) if x is not None else None


def test_capacity_and_sizes_only_host(ctx):
    lib, h = ctx.lib, ctx.handle
    t = _text(0xC801, 3000, 4)
    tb = np.frombuffer(t, np.uint8)
    n = len(tb)
    for kind in KINDS:
        cov = R.cover(t, 6, 2, kind)
        ws, wl, covered = R.spans(cov)
        z = len(ws)
        assert 2 <= z < n and 0 < covered < n
        ns, cv = C.c_uint64(0), C.c_uint64(0)       # sizes only
        assert lib.tc_repeat_spans(h, _p(tb), n, 6, 2, kind, None, None, _ref(ns), _ref(cv)) == 0 and (ns.value, cv.value) == (z, covered)
        a, b = np.full(z, 0xDEADBEEF, np.uint32), np.full(z, 0xDEADBEEF, np.uint32)
        ns, cv = C.c_uint64(z - 1), C.c_uint64(0)   # one too few: the count, nothing written
        assert lib.tc_repeat_spans(h, _p(tb), n, 6, 2, kind, _p(a), _p(b), _ref(ns), _ref(cv)) == TC_ERR_CAPACITY
        assert (ns.value, cv.value) == (z, covered) and (a == 0xDEADBEEF).all() and (b == 0xDEADBEEF).all()
        ns = C.c_uint64(z)                          # exactly enough; covered = NULL
        assert lib.tc_repeat_spans(h, _p(tb), n, 6, 2, kind, _p(a), _p(b), _ref(ns), None) == 0 and ns.value == z
        assert (a.tolist(), b.tolist()) == (ws.tolist(), wl.tolist())
        a2, b2 = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32)
        ns = C.c_uint64(n)                          # n, always enough: nothing behind the count is written
        assert lib.tc_repeat_spans(h, _p(tb), n, 6, 2, kind, _p(a2), _p(b2), _ref(ns), None) == 0 and ns.value == z
        assert (a2[:z].tolist(), b2[:z].tolist()) == (ws.tolist(), wl.tolist()) and (a2[z:] == 0xDEADBEEF).all() and (b2[z:] == 0xDEADBEEF).all()
        # the dedup: sizes only, one byte too few, exactly enough, covered = NULL
        keep = n - covered
        no, cv = C.c_uint64(0), C.c_uint64(0)
        assert lib.tc_repeat_dedup(h, _p(tb), n, 6, 2, kind, None, _ref(no), _ref(cv)) == 0 and (no.value, cv.value) == (keep, covered)
        out = np.full(keep + 8, 0xEE, np.uint8)
        no, cv = C.c_uint64(keep - 1), C.c_uint64(0)
        assert lib.tc_repeat_dedup(h, _p(tb), n, 6, 2, kind, _p(out), _ref(no), _ref(cv)) == TC_ERR_CAPACITY
        assert (no.value, cv.value) == (keep, covered) and (out == 0xEE).all()
        no = C.c_uint64(keep)
        assert lib.tc_repeat_dedup(h, _p(tb), n, 6, 2, kind, _p(out), _ref(no), None) == 0 and no.value == keep
        assert out[:keep].tobytes() == R.dedup(t, cov) and (out[keep:] == 0xEE).all()
        m = np.full(n, 0xEE, np.uint8)              # the mask with covered = NULL
        assert lib.tc_repeat_mask(h, _p(tb), n, 6, 2, kind, None, _p(m), None) == 0 and m.tolist() == R.mask(t, cov).tolist()


def test_capacity_and_sizes_only_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = _text(0xC802, 3000, 4)
    n = len(t)
    cov = R.cover(t, 6, 2, R.LATER)
    ws, wl, covered = R.spans(cov)
    z, keep = len(ws), n - covered
    d_text = _dev(t)
    a, b = (torch.full((z,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    out = torch.full((keep + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    d_len = ctx.lpf_array_dev(d_text, src=False)[0]
    torch.cuda.synchronize()
    pt, pa, pb, po, pl = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b, out, d_len))
    for name, head in (("tc_repeat_spans_dev", (pt, n, 6, 2, R.LATER)), ("tc_cover_spans_dev", (pl, n, 6))):
        fn = getattr(lib, name)
        a.fill_(-1), b.fill_(-1)
        torch.cuda.synchronize()
        ns, cv = C.c_uint64(0), C.c_uint64(0)
        assert fn(h, *head, None, None, _ref(ns), _ref(cv)) == 0 and (ns.value, cv.value) == (z, covered)
        ns, cv = C.c_uint64(z - 1), C.c_uint64(0)
        assert fn(h, *head, pa, pb, _ref(ns), _ref(cv)) == TC_ERR_CAPACITY and (ns.value, cv.value) == (z, covered)
        assert bool((a == -1).all()) and bool((b == -1).all())
        ns = C.c_uint64(z)
        assert fn(h, *head, pa, pb, _ref(ns), None) == 0 and ns.value == z
        assert (_np(a).tolist(), _np(b).tolist()) == (ws.tolist(), wl.tolist())
    for name, head in (("tc_repeat_dedup_dev", (pt, n, 6, 2, R.LATER)), ("tc_cover_dedup_dev", (pl, pt, n, 6))):
        fn = getattr(lib, name)
        out.fill_(0xEE)
        torch.cuda.synchronize()
        no, cv = C.c_uint64(0), C.c_uint64(0)
        assert fn(h, *head, None, _ref(no), _ref(cv)) == 0 and (no.value, cv.value) == (keep, covered)
        no, cv = C.c_uint64(keep - 1), C.c_uint64(0)
        assert fn(h, *head, po, _ref(no), _ref(cv)) == TC_ERR_CAPACITY and (no.value, cv.value) == (keep, covered)
        assert bool((out == 0xEE).all())
        no = C.c_uint64(keep)
        assert fn(h, *head, po, _ref(no), None) == 0 and no.value == keep
        assert _np(out[:keep]).tobytes() == R.dedup(t, cov) and bool((out[keep:] == 0xEE).all())
    _same_spans(ctx.repeat_spans_dev(d_text, 6, 2, R.LATER, cap=1), (ws, wl, covered), "the retry loop")
    _same_bytes(ctx.repeat_dedup_dev(d_text, 6, 2, R.LATER, cap=1), R.dedup(t, cov), covered, "the retry loop, dedup")
    _same_bytes(ctx.repeat_dedup_dev(d_text, 6, 2, R.LATER, cap=n), R.dedup(t, cov), covered, "capacity n, dedup")
    m = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.tc_repeat_mask_dev(h, pt, n, 6, 2, R.LATER, None, C.c_void_p(m.data_ptr()), None) == 0
    assert _np(m).tolist() == R.mask(t, cov).tolist()
    assert lib.tc_cover_mask_dev(h, pl, None, n, 6, None, C.c_void_p(m.data_ptr()), None) == 0
    assert _np(m).tolist() == R.mask(t, cov).tolist()


def test_bad_arguments(ctx):
    """every TC_ERR_ARG case, before a buffer is touched"""
    import torch
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabra abracadabra", np.uint8).copy()
    n = len(tb)
    a, b = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32)
    out = np.full(n, 0xEE, np.uint8)
    m = LOWER.copy()
    d_text, d_out = _dev(tb), torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_a, d_b = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d_len = torch.full((n,), 3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for dev in (False, True):
        sfx = "_dev" if dev else ""
        text, o = (C.c_void_p(d_text.data_ptr()), C.c_void_p(d_out.data_ptr())) if dev else (_p(tb), _p(out))
        sa, sb = (C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr())) if dev else (_p(a), _p(b))
        spans, mask, dedup = (getattr(lib, "tc_repeat_%s%s" % (w, sfx)) for w in ("spans", "mask", "dedup"))
        for n_, L, q, kind in ((TC_MAX_N + 1, 2, 2, 0), (n, 0, 2, 0), (n, 2, 1, 0), (n, 2, 0, 0), (n, 2, 2, 2), (n, 2, 2, 0xffffffff)):
            ns, no = C.c_uint64(n), C.c_uint64(n)
            assert spans(h, text, n_, L, q, kind, sa, sb, _ref(ns), None) == TC_ERR_ARG
            assert spans(h, text, n_, L, q, kind, None, None, _ref(C.c_uint64(0)), None) == TC_ERR_ARG      # in the sizes-only form too
            assert mask(h, text, n_, L, q, kind, _p(m), o, None) == TC_ERR_ARG
            assert dedup(h, text, n_, L, q, kind, o, _ref(no), None) == TC_ERR_ARG
        ns, no = C.c_uint64(n), C.c_uint64(n)
        assert spans(None, text, n, 2, 2, 0, sa, sb, _ref(ns), None) == TC_ERR_ARG         # a null context
        assert spans(h, None, n, 2, 2, 0, sa, sb, _ref(ns), None) == TC_ERR_ARG            # a null text
        assert spans(h, text, n, 2, 2, 0, sa, sb, None, None) == TC_ERR_ARG                # a null count
        assert spans(h, text, n, 2, 2, 0, None, sb, _ref(ns), None) == TC_ERR_ARG and spans(h, text, n, 2, 2, 0, sa, None, _ref(ns), None) == TC_ERR_ARG
        assert spans(h, text, n, 2, 2, 0, None, None, _ref(C.c_uint64(n)), None) == TC_ERR_ARG     # a capacity without buffers
        assert mask(h, None, n, 2, 2, 0, None, o, None) == TC_ERR_ARG and mask(h, text, n, 2, 2, 0, None, None, None) == TC_ERR_ARG
        assert dedup(h, None, n, 2, 2, 0, o, _ref(no), None) == TC_ERR_ARG and dedup(h, text, n, 2, 2, 0, o, None, None) == TC_ERR_ARG
        assert dedup(h, text, n, 2, 2, 0, None, _ref(C.c_uint64(n)), None) == TC_ERR_ARG
        # out overlapping the text: the same bytes, and a tail of the text
        base = d_text.data_ptr() if dev else tb.ctypes.data
        for off in (0, n - 1):
            assert mask(h, text, n, 2, 2, 0, None, C.c_void_p(base + off), None) == TC_ERR_ARG
            assert dedup(h, text, n, 2, 2, 0, C.c_void_p(base + off), _ref(C.c_uint64(n)), None) == TC_ERR_ARG
        ns, cv = C.c_uint64(5), C.c_uint64(9)       # n = 0: nothing read, no span
        assert spans(h, None, 0, 2, 2, 0, sa, sb, _ref(ns), _ref(cv)) == 0 and (ns.value, cv.value) == (0, 0)
        assert mask(h, None, 0, 2, 2, 0, None, None, None) == 0
        no = C.c_uint64(5)
        assert dedup(h, None, 0, 2, 2, 0, o, _ref(no), None) == 0 and no.value == 0
    pl, pt, po = (C.c_void_p(x.data_ptr()) for x in (d_len, d_text, d_out))
    pa, pb = C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr())
    ns, no = C.c_uint64(n), C.c_uint64(n)
    for n_, L in ((TC_MAX_N + 1, 2), (n, 0)):
        assert lib.tc_cover_spans_dev(h, pl, n_, L, pa, pb, _ref(ns), None) == TC_ERR_ARG
        assert lib.tc_cover_mask_dev(h, pl, pt, n_, L, None, po, None) == TC_ERR_ARG
        assert lib.tc_cover_dedup_dev(h, pl, pt, n_, L, po, _ref(no), None) == TC_ERR_ARG
    assert lib.tc_cover_spans_dev(None, pl, n, 2, pa, pb, _ref(ns), None) == TC_ERR_ARG
    assert lib.tc_cover_spans_dev(h, None, n, 2, pa, pb, _ref(ns), None) == TC_ERR_ARG
    assert lib.tc_cover_spans_dev(h, pl, n, 2, pa, pb, None, None) == TC_ERR_ARG
    assert lib.tc_cover_spans_dev(h, pl, n, 2, pa, None, _ref(ns), None) == TC_ERR_ARG
    assert lib.tc_cover_mask_dev(h, None, pt, n, 2, None, po, None) == TC_ERR_ARG
    assert lib.tc_cover_mask_dev(h, pl, pt, n, 2, None, None, None) == TC_ERR_ARG
    assert lib.tc_cover_mask_dev(h, pl, None, n, 2, _p(m), po, None) == TC_ERR_ARG         # a NULL d_text with a non-NULL map
    assert lib.tc_cover_mask_dev(h, pl, pt, n, 2, None, pt, None) == TC_ERR_ARG            # out overlapping the text
    assert lib.tc_cover_dedup_dev(h, pl, None, n, 2, po, _ref(no), None) == TC_ERR_ARG
    assert lib.tc_cover_dedup_dev(h, None, pt, n, 2, po, _ref(no), None) == TC_ERR_ARG
    assert lib.tc_cover_dedup_dev(h, pl, pt, n, 2, po, None, None) == TC_ERR_ARG
    assert lib.tc_cover_dedup_dev(h, pl, pt, n, 2, C.c_void_p(d_text.data_ptr() + 3), _ref(C.c_uint64(n)), None) == TC_ERR_ARG
    ns = C.c_uint64(5)
    assert lib.tc_cover_spans_dev(h, None, 0, 2, pa, pb, _ref(ns), None) == 0 and ns.value == 0
    torch.cuda.synchronize()
    assert (a == 0xDEADBEEF).all() and (b == 0xDEADBEEF).all() and (out == 0xEE).all()
    assert bool((d_a == -1).all()) and bool((d_b == -1).all()) and bool((d_out == 0xEE).all())
    assert tb.tobytes() == b"abracadabra abracadabra" and _np(d_text).tobytes() == tb.tobytes()
    with pytest.raises(Exception):
        ctx.repeat_spans(b"abcabc", 0)
    with pytest.raises(Exception):
        ctx.repeat_spans(b"abcabc", 2, 1)
    with pytest.raises(Exception):
        ctx.repeat_mask(b"abcabc", 2, 2, 7)
    with pytest.raises(ValueError):
        ctx.repeat_mask(b"abcabc", 2, map=b"short")
    # min_len > n through the text calls: the mask is the text (zeroes without a map), the dedup is the text, nothing sorted
    assert ctx.repeat_mask(b"abcabc", 7, map=LOWER)[0].tobytes() == b"abcabc" and ctx.repeat_mask(b"abcabc", 7)[0].tolist() == [0] * 6
    assert ctx.repeat_dedup(b"abcabc", 7)[0].tobytes() == b"abcabc" and ctx.repeat_dedup(b"abcabc", 7)[1] == 0
    d6 = _dev(b"abcabc")
    assert _np(ctx.repeat_mask_dev(d6, 7, map=LOWER)[0]).tobytes() == b"abcabc" and _np(ctx.repeat_mask_dev(d6, 7)[0]).tolist() == [0] * 6
    assert _np(ctx.repeat_dedup_dev(d6, 7)[0]).tobytes() == b"abcabc"
    no = C.c_uint64(5)                              # ... under the capacity protocol
    assert lib.tc_repeat_dedup(h, _p(tb), n, n + 1, 2, 0, _p(out), _ref(no), None) == TC_ERR_CAPACITY and no.value == n
    assert (out == 0xEE).all()


def test_repeats_before_and_after_on_the_shared_workspace(ctx):
    """the calls share the context's workspace with tc_repeats: neither leaves anything the other trips over"""
    import rep_ref
    t = _text(0xC901, 2000, 4)
    want = rep_ref.repeats(t, rep_ref.MAXIMAL)
    before = ctx.repeats(t, with_sa=True)
    for kind in KINDS:
        _every_way(ctx, t, 5, 2, kind, "between two repeats calls")
        _every_way(ctx, _text(0xC902, 5000, 3), 8, 3, kind, "a larger text")
    _general(ctx, np.full(3 * T, 2, np.uint32), 2, "the general form between them")
    after = ctx.repeats(t, with_sa=True)
    for g1, g2, w in zip(before, after, want):
        assert np.array_equal(g1, w) and np.array_equal(g2, w)


# ------------------------------------------------------------------------------------------------ larger texts
def _mutated_copy(seed, n):
    """a text and, behind it, its copy with a substitution every few hundred bytes"""
    half = np.frombuffer(_text(seed, n // 2, 4), np.uint8)
    copy = half.copy()
    rng = np.random.default_rng(seed + 1)
    at = rng.choice(len(copy), len(copy) // 300, replace=False)
    copy[at] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), copy[at]) + 1) % 4]
    return np.concatenate((half, copy)).tobytes()


@pytest.fixture(scope="module", params=["random", "mutated copy"])
def large(request):
    n = 270000
    t = _text(0xCA00, n, 4) if request.param == "random" else _mutated_copy(0xCA10, n)
    assert len(t) == n
    return t


def test_large_later_is_the_cover_of_the_lpf_array(ctx, large):
    d_text = _dev(large)
    d_lpf = ctx.lpf_array_dev(d_text, src=False)[0]
    for L in (8, 12, 20):
        got = ctx.repeat_spans_dev(d_text, L, 2, R.LATER)
        want = ctx.cover_spans_dev(d_lpf, L)
        assert got[2] == want[2] and _np(got[0]).tolist() == _np(want[0]).tolist() and _np(got[1]).tolist() == _np(want[1]).tolist()
        assert len(got[0]) > 0 or L == 20           # (random bytes over four letters repeat no 20-mer at this length)
        _same_spans(got, R.spans(R.cover_of_len(_np(d_lpf), L)), "L = %d" % L)
        out, covered = ctx.repeat_dedup_dev(d_text, L, 2, R.LATER)
        assert covered == got[2] and out.numel() == len(large) - covered
        _same_bytes((out, covered), R.dedup(large, R.cover_of_len(_np(d_lpf), L)), got[2], "dedup, L = %d" % L)


def test_large_all_at_two_is_read_off_the_unique_prefixes(ctx, large):
    d_text = _dev(large)
    n = len(large)
    up = _np(ctx.unique_prefixes_dev(d_text)).astype(np.int64)
    i = np.arange(n)
    for L in (8, 12, 20):
        ln = np.where((i + L <= n) & ((up == 0) | (up > L)), L, 0)
        want = R.cover_of_len(ln, L)
        out, covered = ctx.repeat_mask_dev(d_text, L, 2, R.ALL, None)
        _same_bytes((out, covered), R.mask(large, want), int(want.sum()), "L = %d" % L)
        dd, c2 = ctx.repeat_dedup_dev(d_text, L, 2, R.ALL)
        assert c2 == covered and dd.numel() == n - covered
        _same_bytes((dd, c2), R.dedup(large, want), covered, "dedup, L = %d" % L)


def test_large_all_at_three_is_the_frequent_kmers(ctx, large):
    d_text = _dev(large)
    n = len(large)
    for L in (8, 11):
        pos, occ, row, sa = (_np(x).astype(np.int64) for x in ctx.kmers_dev(d_text, L, 3, 0, with_sa=True))
        ln = np.zeros(n, np.int64)
        rows = np.repeat(row, occ) + (np.arange(int(occ.sum())) - np.repeat(np.cumsum(occ) - occ, occ))
        ln[sa[rows]] = L
        want = R.cover_of_len(ln, L)
        assert 0 < int(want.sum()) and (int(want.sum()) < n or L == 8)       # (at 8 every byte lies in a frequent 8-mer)
        out, covered = ctx.repeat_mask_dev(d_text, L, 3, R.ALL, None)
        _same_bytes((out, covered), R.mask(large, want), int(want.sum()), "L = %d" % L)
        lo, c2 = ctx.repeat_mask_dev(d_text, L, 3, R.ALL, LOWER)
        _same_bytes((lo, c2), R.mask(large, want, LOWER), covered, "lower case, L = %d" % L)


def test_large_text_cover_is_the_cover_of_the_matching_statistics(ctx, large):
    n = len(large)
    query, target = large[n // 2:n // 2 + 90000], large[:n // 2]
    ms_len = ctx.text_match_stats(query, target, pos=False, occ=False)[0]
    for L in (10, 16, 30):
        want = R.spans(R.cover_of_len(ms_len, L))
        _same_spans(ctx.text_cover_dev(_dev(query), _dev(target), L), want, "text_cover_dev, L = %d" % L)
