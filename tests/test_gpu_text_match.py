"""One text against another on the device (tc_text_match_stats, tc_text_mems, tc_text_lcs, their _dev forms and
tc_mems_from_stats_dev) against the reference of tests/textmatch_ref.py (brute force by bytes.find where that is
affordable, the definitions on a naive enhanced suffix array of Q T otherwise; tests/test_textmatch_ref.py holds the two to
each other).  Everything is compared exactly -- the three arrays with ms_pos / ms_occ given and NULL, the MEM lists, the
LCS and the sum -- through the host and the _dev entries, on the smallest shapes at which the kernels can go wrong: the
pairs whose match would run over the query's end into the target's head (the clamp), a nearest T row thousands of rows
away, row counts on both sides of a group of the min tree at the default fan-out and at fan-out 4, b >> a and a >> b, all
256 byte values, no common byte, Q = T through one pointer, and the capacity / sizes-only / error protocol.  Three levels of
the fan-out-64 tree are out of brute force's reach: there the library's older path -- tc_fm_build_lcp(T) and
tc_fm_match_stats with Q as one pattern -- is the reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classgen
import kmer_ref
import lz_ref
import textmatch_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "text-compression_amd", "csrc", "tc_tm.hpp")).read()
TM_TILE = int(re.search(r"#define TM_NT (\d+)", _SRC).group(1)) * int(re.search(r"#define TM_ITEMS (\d+)", _SRC).group(1))
MIN_LENS = (1, 2, 8)
POISON = 0xDEADBEEF


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(q, t):
    """(ms_len, ms_pos, ms_occ) of a pair, computed once"""
    key = (bytes(q), bytes(t))
    if key not in _REF:
        _REF[key] = R.stats(*key)
    return _REF[key]


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _np32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()


def _same(got, want, what, names=("ms_len", "ms_pos", "ms_occ")):
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        assert g.dtype == np.uint32 and len(g) == len(w), (what, name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s[%d] = %d, want %d" % (what, name, bad[0], g[bad[0]], w[bad[0]])


def _every_way(ctx, q, t, what="", min_lens=MIN_LENS):
    """the statistics with ms_pos / ms_occ given and NULL, the MEMs and the LCS, through the host and the _dev entries"""
    q, t = bytes(q), bytes(t)
    want = _ref(q, t)
    tag = "%s a=%d b=%d" % (what, len(q), len(t))
    d_q, d_t = _dev(q), _dev(t)
    for pos, occ in ((True, True), (False, False), (True, False), (False, True)):
        got = ctx.text_match_stats(q, t, pos=pos, occ=occ)
        assert (got[1] is None) == (not pos) and (got[2] is None) == (not occ)
        _same(got, want, tag + " host pos=%d occ=%d" % (pos, occ))
        got = ctx.text_match_stats_dev(d_q, d_t, pos=pos, occ=occ)
        assert (got[1] is None) == (not pos) and (got[2] is None) == (not occ)
        _same(tuple(_np32(x) if x is not None else None for x in got), want, tag + " dev pos=%d occ=%d" % (pos, occ))
    for min_len in min_lens:
        mems = R.mems_of(want[0], want[1], min_len)
        assert ctx.text_mem_count(q, t, min_len) == len(mems[0]), tag
        _same(ctx.text_mems(q, t, min_len), mems, tag + " host min_len=%d" % min_len, ("mem_start", "mem_pos", "mem_len"))
        _same(tuple(_np32(x) for x in ctx.text_mems_dev(d_q, d_t, min_len)), mems, tag + " dev min_len=%d" % min_len,
              ("mem_start", "mem_pos", "mem_len"))
    lcs = R.lcs_of(want[0], want[1])
    assert ctx.text_lcs(q, t) == lcs, tag
    assert ctx.text_lcs_dev(d_q, d_t) == lcs, tag
    return want


# ------------------------------------------------------------------------------------------------ 1: examples and tiny pairs
def test_the_examples_of_the_header(ctx):
    for q, t, ms_len, ms_pos, ms_occ, mems in R.EXAMPLES:
        want = _every_way(ctx, q, t, repr((q, t)))
        assert (want[0].tolist(), want[1].tolist(), want[2].tolist()) == (ms_len, ms_pos, ms_occ)
        start, pos, ln = ctx.text_mems(q, t, 1)
        assert list(zip(start.tolist(), pos.tolist(), ln.tolist())) == mems
    assert ctx.text_lcs(b"banana", b"ananas") == (5, 1, 0, 15)
    assert ctx.text_lcs(b"ab", b"abab") == (2, 0, 2, 3)
    assert ctx.text_lcs(b"aaaaa", b"aaa") == (3, 0, 0, 12)


def test_tiny_pairs_and_empty_sides(ctx):
    for q in (b"", b"a", b"b", b"aa", b"ab", b"ba"):
        for t in (b"", b"a", b"b", b"aa", b"ab", b"ba"):
            _every_way(ctx, q, t, repr((q, t)))
    assert ctx.text_mem_count(b"", b"abc") == 0 and ctx.text_mem_count(b"abc", b"") == 0
    assert ctx.text_lcs(b"", b"abc") == (0, 0, 0, 0) and ctx.text_lcs(b"abc", b"") == (0, 0, 0, 0)
    assert [x.tolist() for x in ctx.text_match_stats(b"abc", b"")] == [[0, 0, 0]] * 3


# ------------------------------------------------------------------------------------------------ 2: the clamp
def test_matches_that_would_run_over_the_querys_end(ctx):
    want = _every_way(ctx, b"ab", b"abab", "ab / abab")
    assert want[0].tolist() == [2, 1]               # (4 and 3 in Q T without the clamp)
    for k, m in ((3, 7), (7, 3), (40, 41), (41, 40), (100, 1000), (1000, 100)):
        want = _every_way(ctx, b"ab" * k, b"ab" * m, "(ab)^%d / (ab)^%d" % (k, m))
        assert int(want[0][0]) == 2 * min(k, m)


def test_nearest_t_row_thousands_of_rows_away(ctx):
    """unary Q against b aaa: every Q row's upper T neighbour is row 3 and its lower one the last row, across scan tiles
    and tree groups; and the two swapped"""
    q, t = b"a" * 5000, b"b" + b"aaa"
    want = _every_way(ctx, q, t, "a^5000 / baaa")
    assert want[0].tolist() == [3] * 4998 + [2, 1] and want[1].tolist() == [1] * 4998 + [2, 3]
    want = _every_way(ctx, t, q, "baaa / a^5000")
    assert want[0].tolist() == [0, 3, 2, 1] and want[2].tolist() == [0, 4998, 4999, 5000]


# ------------------------------------------------------------------------------------------------ 3: Q = T
def test_same_text_through_one_pointer(ctx):
    rng = np.random.default_rng(0x7301)
    t = rng.permutation(256).astype(np.uint8).tobytes()         # no byte twice: the text has no repeats
    d = _dev(t)
    a = len(t)
    ms_len, ms_pos, ms_occ = (_np32(x) for x in ctx.text_match_stats_dev(d, d))
    assert ms_len.tolist() == [a - i for i in range(a)] and ms_pos.tolist() == list(range(a)) and ms_occ.tolist() == [1] * a
    assert ctx.text_lcs_dev(d, d) == (a, 0, 0, a * (a + 1) // 2)
    start, pos, ln = (_np32(x) for x in ctx.text_mems_dev(d, d))
    assert (start.tolist(), pos.tolist(), ln.tolist()) == ([0], [0], [a])
    t = R.random_text(0x7302, 3000, 2)                          # with repeats: ms_len = a - i all the same
    d = _dev(t)
    got = tuple(_np32(x) for x in ctx.text_match_stats_dev(d, d))
    assert got[0].tolist() == [len(t) - i for i in range(len(t))]
    _same(got, _ref(t, t), "Q = T, 2 letters")
    q, tt = d[100:], d[:2000]                                   # two views of one buffer that overlap
    _same(tuple(_np32(x) for x in ctx.text_match_stats_dev(q, tt)), _ref(t[100:], t[:2000]), "overlapping views")


# ------------------------------------------------------------------------------------------------ 4: row counts
@pytest.mark.parametrize("rows", [63, 64, 65, 4095, 4096, 4097])
def test_random_pairs_at_group_boundaries(ctx, rows):
    """a + b + 1 rows on both sides of a group of the default fan-out (64) and of a second-level group (4096), with
    b >> a and a >> b"""
    n = rows - 1
    small = 5 if n < 100 else 37
    for sigma in (2, 4):
        for a in (small, n - small):
            q, t = R.random_text(0x7400 + rows + sigma, a, sigma), R.random_text(0x7480 + rows + sigma, n - a, sigma)
            _every_way(ctx, q, t, "random over %d" % sigma)


@pytest.mark.parametrize("rows", [1025, 4097])
def test_fanout_4(ctx, rows):
    """trees of 5 and 6 levels, on random pairs and on the pairs whose nearest T rows are far"""
    n = rows - 1
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        for sigma in (2, 4):
            for a in (37, n - 37):
                q, t = R.random_text(0x7500 + rows + sigma, a, sigma), R.random_text(0x7580 + rows + sigma, n - a, sigma)
                _every_way(ctx, q, t, "random over %d, fan-out 4" % sigma)
        _every_way(ctx, b"a" * (n - 4), b"baaa", "unary, fan-out 4")
        _every_way(ctx, b"baaa", b"a" * (n - 4), "unary swapped, fan-out 4")
        _every_way(ctx, b"ab" * (n // 4 - 9), b"ab" * (n // 4 + 9), "period 2, fan-out 4")
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0


# ------------------------------------------------------------------------------------------------ 5, 6: alphabets
def test_all_256_byte_values(ctx):
    rng = np.random.default_rng(0x7601)
    q = bytes(range(0, 256, 2)) + rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    t = bytes(range(255, 0, -2)) + rng.integers(0, 256, 500, dtype=np.uint8).tobytes() + q[40:90]
    assert len(set(q + t)) == 256
    want = _every_way(ctx, q, t, "256 byte values")
    assert int(want[0].max()) >= 50


def test_no_common_byte(ctx):
    q, t = R.random_text(0x7602, 700, 4), bytes(rng_b + 128 for rng_b in R.random_text(0x7603, 900, 4))
    want = _every_way(ctx, q, t, "no common byte")
    assert not want[0].any() and not want[1].any() and not want[2].any()
    assert ctx.text_mem_count(q, t) == 0 and ctx.text_lcs(q, t) == (0, 0, 0, 0)
    assert all(len(x) == 0 for x in ctx.text_mems(q, t))


# ------------------------------------------------------------------------------------------------ 7: three tree levels
@pytest.mark.parametrize("kind", ["genome", "two letters"])
def test_three_tree_levels_against_the_fm_index_path(ctx, kind):
    """a = 70 000, b = 200 000: more than 64^3 rows.  (ms_len, ms_pos + 1, ms_occ) is what tc_fm_match_stats answers for
    the one pattern Q on an index of T with the LCP part"""
    a, b = 70000, 200000
    assert a + b + 1 > 64 ** 3
    if kind == "genome":
        x = classgen.genome_like(a + b, seed=0x7701).tobytes()
        q, t = x[b:], x[:b]
    else:
        q, t = R.random_text(0x7702, a, 2), R.random_text(0x7703, b, 2)
    fm = ctx.fm_build(t, lcp=True)
    try:
        f_len, f_pos, f_occ = fm.match_stats([q])
    finally:
        fm.close()
    assert int(f_len.max()) >= 12
    want = (f_len.astype(np.uint32), (f_pos - (f_len > 0)).astype(np.uint32), f_occ.astype(np.uint32))
    _same(ctx.text_match_stats(q, t), want, kind + " host")
    d_q, d_t = _dev(q), _dev(t)
    d_len, d_pos, d_occ = ctx.text_match_stats_dev(d_q, d_t)
    _same((_np32(d_len), _np32(d_pos), _np32(d_occ)), want, kind + " dev")
    _same((_np32(ctx.text_match_stats_dev(d_q, d_t, pos=False, occ=False)[0]),), want[:1], kind + " dev, ms_len alone")
    for min_len in (1, 12):
        mems = R.mems_of(want[0], want[1], min_len)
        _same(ctx.text_mems(q, t, min_len), mems, kind + " mems", ("mem_start", "mem_pos", "mem_len"))
        _same(tuple(_np32(x) for x in ctx.mems_from_stats_dev(d_len, d_pos, min_len)), mems, kind + " mems from stats",
              ("mem_start", "mem_pos", "mem_len"))
    assert ctx.text_lcs_dev(d_q, d_t) == R.lcs_of(want[0], want[1])


# ------------------------------------------------------------------------------------------------ 8: MEMs
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dp(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def test_mems_capacity_protocol_host(ctx):
    lib, h = ctx.lib, ctx.handle
    q, t = R.random_text(0x7801, 600, 2), R.random_text(0x7802, 900, 2)
    qb, tb = np.frombuffer(q, np.uint8), np.frombuffer(t, np.uint8)
    want = _ref(q, t)
    mems = R.mems_of(want[0], want[1], 2)
    z = len(mems[0])
    assert 2 <= z < len(q)

    def call(s, p, l, cap, min_len=2):
        nmem = C.c_uint64(cap)
        return lib.tc_text_mems(h, _p(qb), len(qb), _p(tb), len(tb), min_len, _p(s), _p(p), _p(l), C.byref(nmem)), nmem.value

    assert call(None, None, None, 0) == (0, z)                  # sizes only
    s, p, l = (np.full(len(q), POISON, np.uint32) for _ in range(3))
    assert call(s, p, l, z - 1) == (TC_ERR_CAPACITY, z)         # one too small: the count, nothing written
    assert all((x == POISON).all() for x in (s, p, l))
    assert call(s, p, l, z) == (0, z)                           # exact
    _same((s[:z], p[:z], l[:z]), mems, "exact capacity", ("mem_start", "mem_pos", "mem_len"))
    assert all((x[z:] == POISON).all() for x in (s, p, l))
    s, p, l = (np.full(len(q), POISON, np.uint32) for _ in range(3))
    assert call(s, p, l, len(q)) == (0, z)                      # capacity a is always enough
    _same((s[:z], p[:z], l[:z]), mems, "capacity a", ("mem_start", "mem_pos", "mem_len"))
    z1 = len(R.mems_of(want[0], want[1], 1)[0])
    assert call(s, p, l, len(q), min_len=1) == (0, z1)


def test_mems_capacity_protocol_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    q, t = R.random_text(0x7803, 600, 2), R.random_text(0x7804, 900, 2)
    want = _ref(q, t)
    mems = R.mems_of(want[0], want[1], 2)
    z = len(mems[0])
    assert 2 <= z < len(q)
    d_q, d_t = _dev(q), _dev(t)
    d_len, d_pos, _ = ctx.text_match_stats_dev(d_q, d_t)

    def calls(s, p, l, cap):
        """the same request to tc_text_mems_dev and to tc_mems_from_stats_dev"""
        torch.cuda.synchronize()
        out = []
        nmem = C.c_uint64(cap)
        out.append((lib.tc_text_mems_dev(h, _dp(d_q), len(q), _dp(d_t), len(t), 2, _dp(s), _dp(p), _dp(l), C.byref(nmem)), nmem.value))
        nmem = C.c_uint64(cap)
        out.append((lib.tc_mems_from_stats_dev(h, _dp(d_len), _dp(d_pos), len(q), 2, _dp(s), _dp(p), _dp(l), C.byref(nmem)), nmem.value))
        return out

    assert calls(None, None, None, 0) == [(0, z)] * 2
    s, p, l = (torch.full((len(q),), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    assert calls(s, p, l, z - 1) == [(TC_ERR_CAPACITY, z)] * 2
    assert all(bool((x == -1).all()) for x in (s, p, l))
    for cap in (z, len(q)):
        assert calls(s, p, l, cap) == [(0, z)] * 2
        _same(tuple(_np32(x[:z]) for x in (s, p, l)), mems, "capacity %d" % cap, ("mem_start", "mem_pos", "mem_len"))
        assert all(bool((x[z:] == -1).all()) for x in (s, p, l))
    res = ctx.text_mems_dev(d_q, d_t, 2, cap=1)                 # the retry loop: a first capacity that is too small
    _same(tuple(_np32(x) for x in res), mems, "retry", ("mem_start", "mem_pos", "mem_len"))


@pytest.mark.parametrize("a", [1, TM_TILE - 1, TM_TILE, TM_TILE + 1, 2 * TM_TILE + 1])
def test_mems_from_stats_on_arrays_no_text_produces(ctx, a):
    """the filter compares and copies: any contents, held to the NumPy restatement of the rule"""
    import torch
    rng = np.random.default_rng(0x7810 + a)
    arrays = {
        "all equal": np.full(a, 5, np.uint32),
        "strictly rising": np.arange(1, a + 1, dtype=np.uint32),
        "strictly falling": np.arange(a + 8, 8, -1, dtype=np.uint32),
        "zeros": np.zeros(a, np.uint32),
        "top bit set": rng.integers(0, 1 << 32, a, dtype=np.uint64).astype(np.uint32) | np.uint32(0x80000000),
    }
    ms_pos = rng.integers(0, 1 << 32, a, dtype=np.uint64).astype(np.uint32)
    d_pos = torch.from_numpy(ms_pos.view(np.int32).copy()).cuda()
    for name, ms_len in arrays.items():
        d_len = torch.from_numpy(ms_len.view(np.int32).copy()).cuda()
        for min_len in MIN_LENS + (0x80000000, 0xffffffff):
            want = R.mems_of(ms_len, ms_pos, min_len)
            got = tuple(_np32(x) for x in ctx.mems_from_stats_dev(d_len, d_pos, min_len))
            _same(got, want, "%s a=%d min_len=%d" % (name, a, min_len), ("mem_start", "mem_pos", "mem_len"))
    assert len(R.mems_of(arrays["all equal"], ms_pos, 1)[0]) == a       # (every position, the first and the last tile's included)
    assert len(R.mems_of(arrays["strictly falling"], ms_pos, 1)[0]) == 1


# ------------------------------------------------------------------------------------------------ 9: errors
def test_bad_arguments_leave_the_outputs_untouched(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    qb, tb = np.frombuffer(b"abracadabra", np.uint8), np.frombuffer(b"cadabraabra", np.uint8)
    a, b = len(qb), len(tb)
    x, y, z = (np.full(a, POISON, np.uint32) for _ in range(3))
    words = [C.c_uint32(7), C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)]

    def stats(q=_p(qb), a=a, t=_p(tb), b=b, ln=_p(x), pos=_p(y), occ=_p(z)):
        return lib.tc_text_match_stats(h, q, a, t, b, ln, pos, occ)

    def mems(q=_p(qb), a=a, t=_p(tb), b=b, min_len=1, s=_p(x), p=_p(y), l=_p(z), cap=a):
        nmem = C.c_uint64(cap) if cap is not None else None
        return lib.tc_text_mems(h, q, a, t, b, min_len, s, p, l, C.byref(nmem) if nmem is not None else None), nmem

    def lcs(q=_p(qb), a=a, t=_p(tb), b=b, drop=None):
        refs = [C.byref(w) if k != drop else None for k, w in enumerate(words)]
        return lib.tc_text_lcs(h, q, a, t, b, *refs)

    assert stats(ln=None) == TC_ERR_ARG and stats(q=None) == TC_ERR_ARG and stats(t=None) == TC_ERR_ARG
    assert stats(a=TC_MAX_N, b=1) == TC_ERR_ARG and stats(a=1, b=TC_MAX_N) == TC_ERR_ARG and stats(a=TC_MAX_N + 1) == TC_ERR_ARG
    assert stats(a=1 << 63, b=1 << 63) == TC_ERR_ARG                        # (a sum that wraps)
    for kw in (dict(min_len=0), dict(q=None), dict(t=None), dict(a=TC_MAX_N, b=1), dict(s=None), dict(p=None), dict(l=None),
               dict(s=None, p=None, l=None), dict(min_len=0, s=None, p=None, l=None, cap=0)):
        rc, nmem = mems(**kw)
        assert rc == TC_ERR_ARG and nmem.value == kw.get("cap", a), kw      # (the capacity word too)
    assert mems(cap=None)[0] == TC_ERR_ARG
    assert lcs(q=None) == TC_ERR_ARG and lcs(t=None) == TC_ERR_ARG and lcs(a=TC_MAX_N, b=1) == TC_ERR_ARG
    for drop in range(4):
        assert lcs(drop=drop) == TC_ERR_ARG
    assert all((v == POISON).all() for v in (x, y, z)) and [w.value for w in words] == [7, 7, 7, 7]
    # the _dev forms and the filter
    d_q, d_t = _dev(qb.tobytes()), _dev(tb.tobytes())
    dx, dy, dz = (torch.full((a,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    assert lib.tc_text_match_stats_dev(h, _dp(d_q), a, _dp(d_t), b, None, _dp(dy), _dp(dz)) == TC_ERR_ARG
    assert lib.tc_text_match_stats_dev(h, None, a, _dp(d_t), b, _dp(dx), _dp(dy), _dp(dz)) == TC_ERR_ARG
    assert lib.tc_text_match_stats_dev(h, _dp(d_q), TC_MAX_N, _dp(d_t), b, _dp(dx), _dp(dy), _dp(dz)) == TC_ERR_ARG
    nmem = C.c_uint64(a)
    assert lib.tc_text_mems_dev(h, _dp(d_q), a, _dp(d_t), b, 0, _dp(dx), _dp(dy), _dp(dz), C.byref(nmem)) == TC_ERR_ARG
    assert lib.tc_mems_from_stats_dev(h, _dp(dx), _dp(dy), a, 0, _dp(dx), _dp(dy), _dp(dz), C.byref(nmem)) == TC_ERR_ARG
    assert lib.tc_mems_from_stats_dev(h, None, _dp(dy), a, 1, _dp(dx), _dp(dy), _dp(dz), C.byref(nmem)) == TC_ERR_ARG
    assert lib.tc_mems_from_stats_dev(h, _dp(dx), _dp(dy), a, 1, _dp(dx), None, _dp(dz), C.byref(nmem)) == TC_ERR_ARG
    assert lib.tc_mems_from_stats_dev(h, _dp(dx), _dp(dy), TC_MAX_N + 1, 1, _dp(dx), _dp(dy), _dp(dz), C.byref(nmem)) == TC_ERR_ARG
    assert lib.tc_mems_from_stats_dev(h, _dp(dx), _dp(dy), a, 1, _dp(dx), _dp(dy), _dp(dz), None) == TC_ERR_ARG
    assert lib.tc_text_lcs_dev(h, _dp(d_q), a, _dp(d_t), b, None, C.byref(words[1]), C.byref(words[2]), C.byref(words[3])) == TC_ERR_ARG
    assert nmem.value == a and all(bool((v == -1).all()) for v in (dx, dy, dz)) and [w.value for w in words] == [7, 7, 7, 7]
    with pytest.raises(Exception):
        ctx.text_mems(b"abc", b"abc", min_len=0)
    # a = 0: TC_OK with nothing read or written; b = 0: zeros, no MEMs
    assert stats(q=None, a=0) == 0 and (x == POISON).all()
    rc, nmem = mems(q=None, a=0)
    assert rc == 0 and nmem.value == 0 and (x == POISON).all()
    assert lcs(q=None, a=0) == 0 and [w.value for w in words] == [0, 0, 0, 0]
    assert stats(t=None, b=0, occ=None) == 0 and not x.any() and not y.any() and (z == POISON).all()
    rc, nmem = mems(t=None, b=0)
    assert rc == 0 and nmem.value == 0 and (z == POISON).all()
    assert lib.tc_text_match_stats_dev(h, _dp(d_q), a, None, 0, _dp(dx), None, _dp(dz)) == 0
    assert not bool(dx.any()) and bool((dy == -1).all()) and not bool(dz.any())
    assert stats() == 0                                                     # and the context still answers
    _same((x, y, z), _ref(qb.tobytes(), tb.tobytes()), "after the errors")


# ------------------------------------------------------------------------------------------------ 10, 11: contexts
def test_two_contexts_interleaved(ctx):
    import textcomp
    q1, t1 = R.random_text(0x7a01, 500, 2), R.random_text(0x7a02, 1500, 2)
    q2, t2 = b"ab" * 400, b"ab" * 300 + R.random_text(0x7a03, 200, 4)
    with textcomp.Context(0) as other:
        assert _dbg(other, "tc_dbg_fm_set_lcp_fanout", 4) == 0          # a setting of one context is not the other's
        a1 = ctx.text_match_stats(q1, t1)
        b2 = other.text_mems(q2, t2, 2)
        b1 = ctx.text_mems(q1, t1, 2)
        a2 = other.text_match_stats(q2, t2)
        c1 = ctx.text_lcs(q1, t1)
        c2 = other.text_lcs(q2, t2)
    w1, w2 = _ref(q1, t1), _ref(q2, t2)
    _same(a1, w1, "ctx")
    _same(a2, w2, "other")
    _same(b1, R.mems_of(w1[0], w1[1], 2), "ctx mems", ("mem_start", "mem_pos", "mem_len"))
    _same(b2, R.mems_of(w2[0], w2[1], 2), "other mems", ("mem_start", "mem_pos", "mem_len"))
    assert c1 == R.lcs_of(w1[0], w1[1]) and c2 == R.lcs_of(w2[0], w2[1])


def test_one_context_between_the_other_esa_calls(ctx):
    """tc_lz_parse, then this, then tc_kmers on one context: each answer as if it ran alone"""
    text = R.random_text(0x7b01, 5000, 4)
    q, t = R.random_text(0x7b02, 1200, 4), text[300:4000]
    ps, pl = ctx.lz_parse(text)
    got = ctx.text_match_stats(q, t)
    kp, ko, kr = ctx.kmers(text, 3)
    ps2, pl2 = ctx.lz_parse(text)
    _same(got, _ref(q, t), "between")
    _same(ctx.text_match_stats(q, t), _ref(q, t), "after")
    want_ps, want_pl = lz_ref.parse(text)
    assert np.array_equal(ps, want_ps) and np.array_equal(pl, want_pl) and np.array_equal(ps2, ps) and np.array_equal(pl2, pl)
    want_row, want_pos, want_occ = kmer_ref.by_esa(*kmer_ref.esa(text), 3)
    assert (kp.tolist(), ko.tolist(), kr.tolist()) == (want_pos, want_occ, want_row)
