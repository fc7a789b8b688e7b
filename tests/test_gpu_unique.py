"""What is unique in a text (tc_unique_prefixes, tc_unique_substrings, tc_shortest_unique and their _dev forms) against the
reference of tests/sus_ref.py (numpy over the suffix array and the LCP array; tests/test_sus_ref.py holds it to brute force over
all substrings).  Everything is compared exactly -- up, the MUS list under its window and in its sizes-only form, the point
answers -- through the host and the _dev entries, on the smallest shapes at which the kernels can go wrong: sizes on both sides of
one and two tiles of every pass and of a group of the min tree at the default fan-out and at fan-out 4, unary texts (one MUS over
every position), every byte once (a MUS at every position), a staircase (more than 64 MUS over one position, the shortest in the
middle, ties), a MUS longer than 64^2 positions, a doubled text (answers that are extensions), the window / capacity / sizes-only
/ error protocol, and one text of 270 001 rows against two checks that need no reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sus_ref as S

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "text-compression_amd", "csrc")
# positions per workgroup of the mark, list and scan passes; rows / positions per workgroup of sus_prefix_kernel and
# sus_point_kernel; entries per workgroup of the list's sum scan
SUS_TILE = int(re.search(r"#define SUS_TILE (\d+)", open(os.path.join(_CSRC, "tc_sus.hpp")).read()).group(1))
ROW_TILE = int(re.search(r"#define FM_MS_NT (\d+)\n#define FM_MS_KERNEL __global__", open(os.path.join(_CSRC, "tc_fm_ms.hpp")).read()).group(1))
_RLE = open(os.path.join(_CSRC, "tc_rle.hpp")).read()
SCAN_TILE = int(re.search(r"#define SCAN_NT (\d+)", _RLE).group(1)) * int(re.search(r"#define SCAN_ITEMS (\d+)", _RLE).group(1))
TILES = sorted({SUS_TILE, ROW_TILE, SCAN_TILE})
TILE_SIZES = sorted({n for T in TILES for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1)})
GROUP_SIZES = [63, 64, 65, 4095, 4096, 4097]


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(t):
    """up, (mus_start, mus_len), (sus_start, sus_len) of a text, computed once and never changed"""
    t = bytes(t)
    if t not in _REF:
        _REF[t] = S.reference(t)
        for a in (_REF[t][0],) + _REF[t][1] + _REF[t][2]:
            a.setflags(write=False)
    return _REF[t]


def _window(mus, min_len, max_len):
    keep = (mus[1] >= min_len) & ((mus[1] <= max_len) if max_len else True)
    return mus[0][keep], mus[1][keep]


def _text(seed, n, sigma):
    rng = np.random.default_rng(seed)
    alpha = (np.arange(sigma) * 256 // sigma).astype(np.uint8)
    return alpha[rng.integers(0, sigma, n)].tobytes()


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _same(got, want, what):
    if not isinstance(got, tuple):
        got, want = (got,), (want,)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint32 and len(g) == len(w), (what, k, g.dtype, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: array %d, [%d] = %d, want %d" % (what, k, bad[0], g[bad[0]], w[bad[0]])


def _host_of(res):
    import torch
    if isinstance(res, torch.Tensor):
        assert res.dtype == torch.int32
        return res.cpu().numpy().astype(np.uint32)
    return tuple(_host_of(r) for r in res)


def _every_way(ctx, t, what="", min_len=1, max_len=0, want=None):
    """the three calls through the host and the _dev entries, and the list's sizes-only form"""
    import torch
    t = bytes(t)
    up, mus, point = want if want is not None else _ref(t)
    mus = _window(mus, min_len, max_len)
    tag = "%s n=%d window=(%d, %d)" % (what, len(t), min_len, max_len)
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    _same(ctx.unique_prefixes(t), up, tag + " up host")
    _same(_host_of(ctx.unique_prefixes_dev(d_text)), up, tag + " up dev")
    assert ctx.unique_substring_count(t, min_len, max_len) == len(mus[0]), tag
    _same(ctx.unique_substrings(t, min_len, max_len), mus, tag + " list host")
    _same(_host_of(ctx.unique_substrings_dev(d_text, min_len, max_len)), mus, tag + " list dev")
    _same(ctx.shortest_unique(t), point, tag + " point host")
    _same(_host_of(ctx.shortest_unique_dev(d_text)), point, tag + " point dev")


def _pairs(a):
    return list(zip(a[0].tolist(), a[1].tolist()))


# ------------------------------------------------------------------------------------------------ texts
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"aa", b"ab", b"ba"):
        _every_way(ctx, t, repr(t))
    assert ctx.unique_substring_count(b"") == 0 and len(ctx.unique_prefixes(b"")) == 0
    assert _pairs(ctx.unique_substrings(b"ab")) == [(0, 1), (1, 1)] and _pairs(ctx.unique_substrings(b"aa")) == [(0, 2)]


def test_worked_examples(ctx):
    table = {
        b"mississippi": ([1, 5, 4, 3, 5, 4, 3, 2, 2, 2, 0], [(0, 1), (3, 3), (7, 2), (8, 2), (9, 2)],
                         [(0, 1), (0, 2), (0, 3), (3, 3), (3, 3), (3, 3), (6, 3), (7, 2), (7, 2), (8, 2), (9, 2)]),
        b"abaab": ([3, 2, 2, 0, 0], [(1, 2), (2, 2)], [(0, 3), (1, 2), (1, 2), (2, 2), (2, 3)]),
        b"banana": ([1, 4, 3, 0, 0, 0], [(0, 1), (2, 3)], [(0, 1), (0, 2), (0, 3), (2, 3), (2, 3), (2, 4)]),
        b"abcabc": ([4, 3, 2, 0, 0, 0], [(2, 2)], [(0, 4), (1, 3), (2, 2), (2, 2), (2, 3), (2, 4)]),
        b"aaaa": ([4, 0, 0, 0], [(0, 4)], [(0, 4)] * 4),
        b"a": ([1], [(0, 1)], [(0, 1)]),
    }
    for t, (up, mus, point) in table.items():
        _every_way(ctx, t, repr(t))
        assert ctx.unique_prefixes(t).tolist() == up and _pairs(ctx.unique_substrings(t)) == mus
        assert _pairs(ctx.shortest_unique(t)) == point


@pytest.mark.parametrize("n", [2, 255, 256, 257])
def test_unary_texts(ctx, n):
    """one MUS, the whole text, over every position; up = 0 everywhere else"""
    t = b"a" * n
    _every_way(ctx, t, "unary")
    assert ctx.unique_prefixes(t).tolist() == [n] + [0] * (n - 1)
    assert _pairs(ctx.unique_substrings(t)) == [(0, n)] and _pairs(ctx.shortest_unique(t)) == [(0, n)] * n
    _every_way(ctx, t, "unary", 1, n - 1)           # the window cuts it
    _every_way(ctx, t, "unary", n, n)               # and keeps it


def test_every_byte_value_once(ctx):
    t = bytes((i * 167 + 13) & 255 for i in range(256))
    assert len(set(t)) == 256
    _every_way(ctx, t, "all bytes")
    assert _pairs(ctx.unique_substrings(t)) == [(p, 1) for p in range(256)]
    assert _pairs(ctx.shortest_unique(t)) == [(p, 1) for p in range(256)]


@pytest.mark.parametrize("n", sorted(set(TILE_SIZES + GROUP_SIZES)))
def test_sizes_at_tile_and_group_boundaries(ctx, n):
    """n on both sides of one and two tiles of every pass (the prefix and point kernels, the mark / list / scan passes, the
    sum scan) and of a group (64) and a second-level group (4096) of the min tree at the default fan-out"""
    for sigma in (2, 4, 96):
        _every_way(ctx, _text(0x5100 + 7 * n + sigma, n, sigma), "random over %d" % sigma)


@pytest.mark.parametrize("n", GROUP_SIZES[:4])
def test_fanout_4(ctx, n):
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        for sigma in (2, 4, 96):
            _every_way(ctx, _text(0x5100 + 7 * n + sigma, n, sigma), "random over %d, fan-out 4" % sigma)
        _every_way(ctx, b"a" * n, "unary, fan-out 4")
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0


def _staircase_properties(t):
    """from the reference alone: (the most MUS over one position, answers that are a covering MUS neither first nor last of
    the covering ones, positions with a tie for the shortest covering MUS, answers that are a covering MUS, a predecessor
    extended right, a successor extended left)"""
    up, (ms, ml), (ss, sl) = _ref(t)
    n = len(t)
    ms64, me64 = ms.astype(np.int64), ms.astype(np.int64) + ml - 1
    p = np.arange(n)
    first = np.searchsorted(me64, p, side="left")           # the covering MUS of p are first .. last
    last = np.searchsorted(ms64, p, side="right") - 1
    at = np.minimum(np.searchsorted(ms64, ss.astype(np.int64)), len(ms) - 1)    # the answer as a MUS index, where it is one
    is_cover = (ms64[at] == ss) & (ml[at] == sl) & (first <= last)
    interior = is_cover & (at > first) & (at < last)
    ties = 0
    for q in np.nonzero(first <= last)[0]:
        lens = ml[first[q]:last[q] + 1]
        if int((lens == lens.min()).sum()) > 1:
            if is_cover[q]:
                assert at[q] == first[q] + int(np.argmin(lens))     # resolved to the left
            ties += 1
    right = (~is_cover) & (ss < p) & (ss.astype(np.int64) + sl - 1 == p)
    left = (~is_cover) & (ss == p)
    assert int(is_cover.sum()) + int(right.sum()) + int(left.sum()) == n
    return int((last - first + 1).max()), int(interior.sum()), ties, int(is_cover.sum()), int(right.sum()), int(left.sum())


@pytest.fixture(scope="module")
def staircase():
    """A = 2 base + steps stride + 8 random ACGT bytes; for k = 0 .. steps - 1 the byte 128 + k % 100 and a copy
    A[k stride : k stride + ln_k], ln_0 = base + steps, ln_k = max(base, ln_(k-1) + randint(-(stride - 1), stride - 1)); the byte
    255 (tests/sus_ref.py: staircase, Python's random.Random(7), base 200, steps 140, stride 4).  The properties the case is
    about are asserted from the reference before any device call: a case that lacks them fails."""
    t = S.staircase(7, 200, 140, 4)
    deepest, interior, ties, cover, right, left = _staircase_properties(t)
    assert deepest >= 65                            # more MUS over one position than a group of the tree holds
    assert interior >= 1                            # a shortest covering MUS that is neither the first nor the last of them
    assert ties >= 1                                # a tie for the minimum, resolved to the left
    assert cover >= 1 and right >= 1 and left >= 1  # all three kinds of answer
    return t


@pytest.mark.parametrize("fanout", [64, 4])
def test_staircase(ctx, staircase, fanout):
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", fanout) == 0
    try:
        _every_way(ctx, staircase, "staircase, fan-out %d" % fanout)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0


@pytest.mark.parametrize("m", [300, 4200])
def test_a_long_mus(ctx, m):
    """a Y b c a Y e f g Y b: a Y b occurs once, a Y and Y b twice -- the MUS (0, |Y| + 2), the answer at p = 0 and, by the tie
    rule, at p = 1; at |Y| = 4200 the range the minimum is taken over spans more than 64^2 positions"""
    Y = bytes(b"ACGT"[c] for c in np.random.default_rng(0x5200 + m).integers(0, 4, m))
    t = b"a" + Y + b"bca" + Y + b"efg" + Y + b"b"
    (ms, ml), (ss, sl) = _ref(t)[1], _ref(t)[2]
    assert (int(ms[0]), int(ml[0])) == (0, m + 2)
    assert (int(ss[0]), int(sl[0])) == (0, m + 2) and (int(ss[1]), int(sl[1])) == (0, m + 2)
    _every_way(ctx, t, "a long MUS")


def test_doubled_text(ctx):
    """X X: every MUS starts in the second copy's neighbourhood, so nearly every answer of the first copy is a successor
    extended left and nearly every one of the second a predecessor extended right; (350, 351) at p = 350"""
    X = bytes(b"ACGT"[c] for c in np.random.default_rng(0x5300).integers(0, 4, 700))
    t = X + X
    ss, sl = _ref(t)[2]
    assert (int(ss[350]), int(sl[350])) == (350, 351)
    assert int((ss == np.arange(len(t))).sum()) >= 690      # (698 of the 700 positions of the first copy)
    _every_way(ctx, t, "doubled")


def test_windows(ctx):
    t = _text(0x5400, 3000, 4)
    ml = _ref(t)[1][1]
    for lo, hi in ((1, 0), (2, 0), (1, 1), (3, 5), (int(ml.max()) + 1, 0), (0xffffffff, 0), (5, 0xffffffff)):
        _every_way(ctx, t, "windows", lo, hi)
    assert 0 < len(_window(_ref(t)[1], 3, 5)[0]) < len(ml) and len(_window(_ref(t)[1], int(ml.max()) + 1, 0)[0]) == 0


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _list(lib, h, name, text, n, min_len, max_len, start, ln, nmus):
    return getattr(lib, name)(h, text, n, min_len, max_len, start, ln, C.byref(nmus) if nmus is not None else None)


def test_capacity_and_sizes_only_host(ctx):
    lib, h = ctx.lib, ctx.handle
    t = _text(0x5501, 400, 3)
    tb = np.frombuffer(t, np.uint8)
    want = _ref(t)[1]
    z = len(want[0])
    assert 2 <= z < len(t)
    nmus = C.c_uint64(0)                            # sizes only
    assert _list(lib, h, "tc_unique_substrings", _p(tb), len(tb), 1, 0, None, None, nmus) == 0 and nmus.value == z
    a, b = np.full(z, 0xDEADBEEF, np.uint32), np.full(z, 0xDEADBEEF, np.uint32)
    nmus = C.c_uint64(z - 1)                        # one too few: the count, nothing written
    assert _list(lib, h, "tc_unique_substrings", _p(tb), len(tb), 1, 0, _p(a), _p(b), nmus) == TC_ERR_CAPACITY and nmus.value == z
    assert (a == 0xDEADBEEF).all() and (b == 0xDEADBEEF).all()
    nmus = C.c_uint64(z)                            # exactly enough
    assert _list(lib, h, "tc_unique_substrings", _p(tb), len(tb), 1, 0, _p(a), _p(b), nmus) == 0 and nmus.value == z
    _same((a, b), want, "exact capacity")
    a2, b2 = np.full(len(t), 0xDEADBEEF, np.uint32), np.full(len(t), 0xDEADBEEF, np.uint32)
    nmus = C.c_uint64(len(t))                       # n, always enough: nothing behind the count is written
    assert _list(lib, h, "tc_unique_substrings", _p(tb), len(tb), 1, 0, _p(a2), _p(b2), nmus) == 0 and nmus.value == z
    _same((a2[:z], b2[:z]), want, "capacity n")
    assert (a2[z:] == 0xDEADBEEF).all() and (b2[z:] == 0xDEADBEEF).all()


def test_capacity_and_sizes_only_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = _text(0x5502, 400, 3)
    want = _ref(t)[1]
    z = len(want[0])
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    a, b = (torch.full((z,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    pt, pa, pb = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b))
    nmus = C.c_uint64(0)
    assert _list(lib, h, "tc_unique_substrings_dev", pt, len(t), 1, 0, None, None, nmus) == 0 and nmus.value == z
    nmus = C.c_uint64(z - 1)
    assert _list(lib, h, "tc_unique_substrings_dev", pt, len(t), 1, 0, pa, pb, nmus) == TC_ERR_CAPACITY and nmus.value == z
    assert bool((a == -1).all()) and bool((b == -1).all())
    nmus = C.c_uint64(z)
    assert _list(lib, h, "tc_unique_substrings_dev", pt, len(t), 1, 0, pa, pb, nmus) == 0 and nmus.value == z
    _same(_host_of((a, b)), want, "exact capacity, dev")
    _same(_host_of(ctx.unique_substrings_dev(d_text, cap=1)), want, "the retry loop")   # a first capacity that is too small
    _same(_host_of(ctx.unique_substrings_dev(d_text, cap=len(t))), want, "capacity n")


def test_bad_arguments_and_edges(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabra", np.uint8)
    n = len(tb)
    up, mus, point = _ref(tb.tobytes())
    z = len(mus[0])
    a, b = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32)

    def call(text=_p(tb), n=n, min_len=1, max_len=0, start=_p(a), ln=_p(b), cap=z, name="tc_unique_substrings"):
        nmus = C.c_uint64(cap) if cap is not None else None
        return _list(lib, h, name, text, n, min_len, max_len, start, ln, nmus), nmus

    for name in ("tc_unique_substrings", "tc_unique_substrings_dev"):   # (argument errors come before any buffer is touched)
        assert call(min_len=0, name=name)[0] == TC_ERR_ARG
        assert call(min_len=5, max_len=4, name=name)[0] == TC_ERR_ARG and call(min_len=3, max_len=2, name=name)[0] == TC_ERR_ARG
        assert call(text=None, name=name)[0] == TC_ERR_ARG
        assert call(n=TC_MAX_N + 1, name=name)[0] == TC_ERR_ARG
        assert call(cap=None, name=name)[0] == TC_ERR_ARG
        assert call(start=None, name=name)[0] == TC_ERR_ARG and call(ln=None, name=name)[0] == TC_ERR_ARG
        assert call(start=None, ln=None, name=name)[0] == TC_ERR_ARG                    # a capacity without buffers
        assert call(min_len=0, start=None, ln=None, cap=0, name=name)[0] == TC_ERR_ARG   # in the sizes-only form too
        rc, nmus = call(text=None, n=0, name=name)                                      # n = 0: nothing read, no MUS
        assert rc == 0 and nmus.value == 0
    for name in ("tc_unique_prefixes", "tc_unique_prefixes_dev"):
        fn = getattr(lib, name)
        assert fn(h, None, n, _p(a)) == TC_ERR_ARG and fn(h, _p(tb), n, None) == TC_ERR_ARG
        assert fn(h, _p(tb), TC_MAX_N + 1, _p(a)) == TC_ERR_ARG
        assert fn(h, None, 0, None) == 0
    for name in ("tc_shortest_unique", "tc_shortest_unique_dev"):
        fn = getattr(lib, name)
        assert fn(h, None, n, _p(a), _p(b)) == TC_ERR_ARG and fn(h, _p(tb), n, _p(a), None) == TC_ERR_ARG
        assert fn(h, _p(tb), TC_MAX_N + 1, _p(a), _p(b)) == TC_ERR_ARG
        assert fn(h, None, 0, None, None) == 0
    assert (a == 0xDEADBEEF).all() and (b == 0xDEADBEEF).all()
    # sus_start alone may be null: it is then not written
    assert lib.tc_shortest_unique(h, _p(tb), n, None, _p(b)) == 0
    _same(b.copy(), point[1], "sus_start = NULL, host")
    d_text = torch.from_numpy(tb.copy()).cuda()
    d_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.tc_shortest_unique_dev(h, C.c_void_p(d_text.data_ptr()), n, None, C.c_void_p(d_len.data_ptr())) == 0
    _same(_host_of(d_len), point[1], "sus_start = NULL, dev")
    rc, nmus = call(min_len=2, max_len=2)
    assert rc == 0 and nmus.value == int((mus[1] == 2).sum())
    with pytest.raises(Exception):
        ctx.unique_substrings(b"abc", min_len=0)
    with pytest.raises(Exception):
        ctx.unique_substrings(b"abc", min_len=4, max_len=3)


def test_repeats_before_and_after_on_the_shared_workspace(ctx):
    """the calls share the context's workspace with tc_repeats: neither leaves anything the other trips over"""
    import rep_ref as R
    t = _text(0x5601, 2000, 4)
    want = R.repeats(t, R.MAXIMAL)
    before = ctx.repeats(t, with_sa=True)
    _every_way(ctx, t, "between two repeats calls")
    _every_way(ctx, _text(0x5602, 5000, 100), "a larger text")
    after = ctx.repeats(t, with_sa=True)
    for g1, g2, w in zip(before, after, want):
        assert np.array_equal(g1, w) and np.array_equal(g2, w)


# ------------------------------------------------------------------------------------------------ one larger text
def test_a_larger_text(ctx):
    """270 000 random ACGT bytes, 270 001 rows: against the reference fed with Context.lcp_array's (sa, lcp), which that call's
    own tests hold, and two checks that need no reference"""
    n = 270000
    t = _text(0x5700, n, 4)
    sa, lcp = ctx.lcp_array(t)
    want = S.from_esa(sa, lcp, n)
    _every_way(ctx, t, "270 000", want=want)
    up = ctx.unique_prefixes(t).astype(np.int64)
    _, unique = ctx.kmer_profile(t, 16)
    i = np.arange(n)
    for k in (8, 12, 16):
        assert int(((up >= 1) & (up <= k) & (i + k <= n)).sum()) == int(unique[k - 1]), k
    sl = ctx.shortest_unique(t)[1].astype(np.int64)
    assert int(np.abs(np.diff(sl)).max()) <= 1
