"""The LPF array, the LZ77 parse of a text against itself and its inverse (tc_lpf_array, tc_lz_parse, tc_lz_unparse and
their _dev forms) against the reference of tests/lz_ref.py (brute force up to 64 bytes, the suffix-array restatement above;
tests/test_lz_ref.py holds the two together).  Everything is compared exactly, through the host and the _dev entries, on the
smallest shapes at which the kernels can go wrong: the group boundaries of the min trees at the default fan-out and at
fan-out 4, texts whose nearest smaller row is far and whose range minima span many groups, tile boundaries of the
phrase-start steps at a tile of 64 positions (tc_dbg_lz_set_tile) and one run at the library's tile, phrase lists no greedy
parser writes, and the capacity / sizes-only / error protocol.  Which tree levels the range minimum reaches cannot be seen
from here: host/check/lz_kernels.cpp (tests/test_host_checks.py) asserts that."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lz_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZ_TILE = int(re.search(r"#define LZ_TILE (\d+)", open(os.path.join(ROOT, "text-compression_amd", "csrc", "tc_lz.hpp")).read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(t):
    """(lpf, src, ph_src, ph_len) of a text, computed once"""
    if t not in _REF:
        lpf, src = R.lpf_src(t)
        _REF[t] = (lpf, src) + R.parse_of(t, lpf, src)
    return _REF[t]


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _np32(t):
    return t.cpu().numpy().astype(np.uint32)


def _every_way(ctx, t, what=""):
    """the LPF array, the parse, the count and the round trip, through the host and the _dev entries"""
    import torch
    t = bytes(t)
    lpf, src, ps, pl = _ref(t)
    got_lpf, got_src = ctx.lpf_array(t)
    bad = np.nonzero((got_lpf != lpf) | (got_src != src))[0]
    assert len(bad) == 0, "%s n=%d: position %d: got (lpf, src) = (%d, %d), want (%d, %d)" % (
        what, len(t), bad[0], got_lpf[bad[0]], got_src[bad[0]], lpf[bad[0]], src[bad[0]])
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    d_lpf, d_src = ctx.lpf_array_dev(d_text)
    assert np.array_equal(_np32(d_lpf), lpf) and np.array_equal(_np32(d_src), src), what
    assert ctx.lz_phrase_count(t) == len(ps), what
    got_ps, got_pl = ctx.lz_parse(t)
    assert got_ps.dtype == np.uint32 and got_pl.dtype == np.uint32
    assert np.array_equal(got_ps, ps) and np.array_equal(got_pl, pl), (what, len(t), got_ps[:8], got_pl[:8], ps[:8], pl[:8])
    d_ps, d_pl = ctx.lz_parse_dev(d_text)
    assert np.array_equal(_np32(d_ps), ps) and np.array_equal(_np32(d_pl), pl), what
    assert ctx.lz_unparse(got_ps, got_pl) == t, what
    assert bytes(ctx.lz_unparse_dev(d_ps, d_pl).cpu().numpy()) == t, what


def _starts(pl):
    return np.concatenate([[0], np.cumsum(np.maximum(pl.astype(np.int64), 1))])


# ------------------------------------------------------------------------------------------------ texts
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"aa", b"ab"):
        _every_way(ctx, t, repr(t))
    assert ctx.lz_phrase_count(b"") == 0
    ps, pl = ctx.lz_parse(b"a" * 64)                # the copy overlaps its own source
    assert ps.tolist() == [97, 0] and pl.tolist() == [0, 63]


def test_structured_texts(ctx):
    _every_way(ctx, b"a" * 64, "unary")
    _every_way(ctx, b"a" * 301, "unary")
    for p in (2, 3, 7):
        _every_way(ctx, R.periodic(100, p), "period %d" % p)
    _every_way(ctx, R.fibonacci(200), "fibonacci")


def test_random_texts(ctx):
    for sigma in (1, 2, 4, 256):
        _every_way(ctx, R.random_text(0x7100 + sigma, 300, sigma), "random over %d" % sigma)


def test_text_followed_by_its_copy_is_one_phrase(ctx):
    half = R.random_text(0x7201, 150, 256)
    t = half + half
    _every_way(ctx, t, "copy")
    ps, pl = ctx.lz_parse(t)
    assert (int(ps[-1]), int(pl[-1])) == (0, 150)


def test_last_byte_new(ctx):
    t = R.random_text(0x7202, 99, 2) + b"z"
    _every_way(ctx, t, "last byte new")
    ps, pl = ctx.lz_parse(t)
    assert (int(ps[-1]), int(pl[-1])) == (ord("z"), 0)


@pytest.mark.parametrize("rows", [63, 64, 65, 4095, 4096, 4097])
def test_row_counts_at_group_boundaries(ctx, rows):
    """N = n + 1 rows on both sides of a group of the default fan-out (64) and of a second-level group (4096)"""
    n = rows - 1
    _every_way(ctx, R.random_text(0x7300 + rows, n, 4), "random, %d rows" % rows)
    _every_way(ctx, b"a" * n, "unary, %d rows" % rows)


@pytest.mark.parametrize("rows", [1025, 4097])
def test_fanout_4(ctx, rows):
    """trees of 5 and 6 levels, on the texts whose nearest smaller row is far and whose range minima span many groups"""
    n = rows - 1
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        _every_way(ctx, b"a" * n, "unary, fan-out 4")
        for p in (2, 3, 7):
            _every_way(ctx, R.periodic(n, p), "period %d, fan-out 4" % p)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0


# ------------------------------------------------------------------------------------------------ tile boundaries
@pytest.fixture
def tile64(ctx):
    assert _dbg(ctx, "tc_dbg_lz_set_tile", 64) == 0
    yield ctx
    assert _dbg(ctx, "tc_dbg_lz_set_tile", 0) == 0


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 1000])
def test_tile_64_sizes(tile64, n):
    _every_way(tile64, R.random_text(0x7400 + n, n, 4), "random, tile 64")
    _every_way(tile64, R.periodic(n, 7), "period 7, tile 64")
    _every_way(tile64, R.random_text(0x7480 + n, n, 256), "bytes, tile 64")


def test_tile_64_phrase_ends_at_a_tile_end(tile64):
    head = R.random_text(0x7501, 32, 256)
    t = head + head + R.random_text(0x7502, 70, 256)
    _, _, ps, pl = _ref(t)
    s = _starts(pl)
    assert any(int(pl[k]) == 32 and int(s[k]) == 32 and int(ps[k]) == 0 for k in range(len(pl)))    # [32, 64)
    _every_way(tile64, t, "phrase ends at a tile end")


def test_tile_64_phrase_skips_three_tiles(tile64):
    r = R.random_text(0x7503, 100, 256)
    t = r + r * 3 + R.random_text(0x7504, 50, 256)
    _, _, ps, pl = _ref(t)
    s = _starts(pl)
    k = int(np.nonzero(s == 100)[0][0])
    assert (int(ps[k]), int(pl[k])) == (0, 300)     # [100, 400): the tiles [128, 192), [192, 256), [256, 320), [320, 384) hold no phrase start
    _every_way(tile64, t, "phrase skips tiles")


def test_tile_64_tiles_of_literals_only(tile64):
    t = bytes(range(256))
    _, _, ps, pl = _ref(t)
    assert not pl.any() and ps.tolist() == list(range(256))
    _every_way(tile64, t, "literals only")


def test_default_tile_two_tiles_and_a_byte(ctx):
    n = 2 * LZ_TILE + 1
    _every_way(ctx, R.periodic(n, 7), "period 7, default tile")
    _every_way(ctx, R.random_text(0x7601, n, 4), "random, default tile")


# ------------------------------------------------------------------------------------------------ lists no greedy parser writes
def _unparse_both(ctx, ps, pl):
    import torch
    ps, pl = np.array(ps, np.uint32), np.array(pl, np.uint32)
    assert R.valid(ps, pl)
    want = R.unparse(ps, pl)
    assert ctx.lz_unparse(ps, pl) == want
    d = ctx.lz_unparse_dev(torch.from_numpy(ps.astype(np.int32)).cuda(), torch.from_numpy(pl.astype(np.int32)).cuda())
    assert bytes(d.cpu().numpy()) == want
    return want


def test_unparse_hand_made_lists(ctx):
    # short copies where longer ones exist
    assert _unparse_both(ctx, [97, 98, 99, 0, 2, 3], [0, 0, 0, 2, 1, 3]) == b"abcabcabc"
    # a copy chain of depth n: every byte copies the one before it
    n = 3000
    assert _unparse_both(ctx, [120] + list(range(n - 1)), [0] + [1] * (n - 1)) == b"x" * n
    # two interleaved chains, and overlapping copies of period 2 on top of them
    ps = [97, 98] + list(range(0, 500)) + [1, 0]
    pl = [0, 0] + [1] * 500 + [700, 3]
    want = _unparse_both(ctx, ps, pl)
    assert len(want) == 2 + 500 + 703 and want[:6] == b"ababab"
    for tile in (64, 0):
        assert _dbg(ctx, "tc_dbg_lz_set_tile", tile) == 0
        t = R.random_text(0x7701, 777, 2)
        assert ctx.lz_unparse(*ctx.lz_parse(t)) == t
    assert ctx.lz_unparse([], []) == b""


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_capacity_and_sizes_only_host(ctx):
    lib, h = ctx.lib, ctx.handle
    t = R.random_text(0x7801, 200, 4)
    tb = np.frombuffer(t, np.uint8)
    _, _, ps, pl = _ref(t)
    z = len(ps)
    nph = C.c_uint64(0)                             # sizes only
    assert lib.tc_lz_parse(h, _p(tb), len(tb), None, None, C.byref(nph)) == 0 and nph.value == z
    a, b = np.full(z, 0xDEADBEEF, np.uint32), np.full(z, 0xDEADBEEF, np.uint32)
    nph = C.c_uint64(z - 1)                         # one too small: the count, nothing written
    assert lib.tc_lz_parse(h, _p(tb), len(tb), _p(a), _p(b), C.byref(nph)) == TC_ERR_CAPACITY and nph.value == z
    assert (a == 0xDEADBEEF).all() and (b == 0xDEADBEEF).all()
    nph = C.c_uint64(z)
    assert lib.tc_lz_parse(h, _p(tb), len(tb), _p(a), _p(b), C.byref(nph)) == 0 and nph.value == z
    assert np.array_equal(a, ps) and np.array_equal(b, pl)
    nb = C.c_uint64(0)                              # the inverse: sizes only, one too small, exact
    assert lib.tc_lz_unparse(h, _p(a), _p(b), z, None, C.byref(nb)) == 0 and nb.value == len(t)
    out = np.full(len(t), 0xEE, np.uint8)
    nb = C.c_uint64(len(t) - 1)
    assert lib.tc_lz_unparse(h, _p(a), _p(b), z, _p(out), C.byref(nb)) == TC_ERR_CAPACITY and nb.value == len(t)
    assert (out == 0xEE).all()
    nb = C.c_uint64(len(t))
    assert lib.tc_lz_unparse(h, _p(a), _p(b), z, _p(out), C.byref(nb)) == 0 and nb.value == len(t) and out.tobytes() == t


def test_capacity_and_sizes_only_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = R.random_text(0x7802, 200, 4)
    _, _, ps, pl = _ref(t)
    z = len(ps)
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    a = torch.full((z,), -1, dtype=torch.int32, device="cuda")
    b = torch.full((z,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pt, pa, pb = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b))
    nph = C.c_uint64(0)
    assert lib.tc_lz_parse_dev(h, pt, len(t), None, None, C.byref(nph)) == 0 and nph.value == z
    nph = C.c_uint64(z - 1)
    assert lib.tc_lz_parse_dev(h, pt, len(t), pa, pb, C.byref(nph)) == TC_ERR_CAPACITY and nph.value == z
    assert bool((a == -1).all()) and bool((b == -1).all())
    nph = C.c_uint64(z)
    assert lib.tc_lz_parse_dev(h, pt, len(t), pa, pb, C.byref(nph)) == 0 and nph.value == z
    assert np.array_equal(_np32(a), ps) and np.array_equal(_np32(b), pl)
    out = torch.full((len(t),), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    po = C.c_void_p(out.data_ptr())
    nb = C.c_uint64(0)
    assert lib.tc_lz_unparse_dev(h, pa, pb, z, None, C.byref(nb)) == 0 and nb.value == len(t)
    nb = C.c_uint64(len(t) - 1)
    assert lib.tc_lz_unparse_dev(h, pa, pb, z, po, C.byref(nb)) == TC_ERR_CAPACITY and nb.value == len(t)
    assert bool((out == 0xEE).all())
    nb = C.c_uint64(len(t))
    assert lib.tc_lz_unparse_dev(h, pa, pb, z, po, C.byref(nb)) == 0 and bytes(out.cpu().numpy()) == t


def test_null_buffers_and_edges(ctx):
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabra", np.uint8)
    n = len(tb)
    a, b = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    nph = C.c_uint64(n)
    assert lib.tc_lpf_array(h, _p(tb), n, None, _p(b)) == TC_ERR_ARG
    assert lib.tc_lpf_array(h, None, n, _p(a), _p(b)) == TC_ERR_ARG
    assert lib.tc_lpf_array(h, _p(tb), TC_MAX_N + 1, _p(a), _p(b)) == TC_ERR_ARG
    assert lib.tc_lpf_array(h, _p(tb), n, _p(a), None) == 0                     # src may be null
    assert a.tolist() == _ref(tb.tobytes())[0].tolist()
    assert lib.tc_lpf_array(h, None, 0, _p(a), _p(b)) == 0                      # n = 0: nothing read
    assert lib.tc_lz_parse(h, _p(tb), n, _p(a), _p(b), None) == TC_ERR_ARG
    assert lib.tc_lz_parse(h, _p(tb), n, None, _p(b), C.byref(nph)) == TC_ERR_ARG
    nph = C.c_uint64(n)
    assert lib.tc_lz_parse(h, _p(tb), n, _p(a), None, C.byref(nph)) == TC_ERR_ARG
    nph = C.c_uint64(n)
    assert lib.tc_lz_parse(h, None, n, _p(a), _p(b), C.byref(nph)) == TC_ERR_ARG
    nph = C.c_uint64(n)
    assert lib.tc_lz_parse(h, _p(tb), TC_MAX_N + 1, _p(a), _p(b), C.byref(nph)) == TC_ERR_ARG
    nph = C.c_uint64(n)
    assert lib.tc_lz_parse(h, None, 0, _p(a), _p(b), C.byref(nph)) == 0 and nph.value == 0
    out = np.zeros(16, np.uint8)
    nb = C.c_uint64(16)
    assert lib.tc_lz_unparse(h, None, _p(b), 1, _p(out), C.byref(nb)) == TC_ERR_ARG
    nb = C.c_uint64(16)
    assert lib.tc_lz_unparse(h, _p(a), None, 1, _p(out), C.byref(nb)) == TC_ERR_ARG
    assert lib.tc_lz_unparse(h, _p(a), _p(b), 1, _p(out), None) == TC_ERR_ARG
    nb = C.c_uint64(16)
    assert lib.tc_lz_unparse(h, _p(a), _p(b), 1, None, C.byref(nb)) == TC_ERR_ARG       # a capacity without a buffer
    nb = C.c_uint64(16)
    assert lib.tc_lz_unparse(h, None, None, 0, _p(out), C.byref(nb)) == 0 and nb.value == 0     # no phrases: no bytes
    for ok in (64, 128, 16384, 0):
        assert _dbg(ctx, "tc_dbg_lz_set_tile", ok) == 0
    for bad in (1, 32, 63, 96, 32768):
        assert _dbg(ctx, "tc_dbg_lz_set_tile", bad) == TC_ERR_ARG


@pytest.mark.parametrize("ps,pl", [([97, 1], [0, 3]),           # a copy whose source is its own start
                                   ([97, 2], [0, 3]),           # ... behind its own start
                                   ([0], [1]),                  # a copy at position 0
                                   ([97, 98, 256], [0, 0, 0]),  # a literal above 255
                                   ([97, 0, 2 ** 32 - 1], [0, 5, 1])])
def test_bad_phrase_lists(ctx, ps, pl):
    import torch
    lib, h = ctx.lib, ctx.handle
    assert not R.valid(ps, pl)
    a, b = np.array(ps, np.uint32), np.array(pl, np.uint32)
    out = np.full(64, 0xEE, np.uint8)
    nb = C.c_uint64(64)
    assert lib.tc_lz_unparse(h, _p(a), _p(b), len(a), _p(out), C.byref(nb)) == TC_ERR_ARG
    assert (out == 0xEE).all()
    nb = C.c_uint64(0)
    assert lib.tc_lz_unparse(h, _p(a), _p(b), len(a), None, C.byref(nb)) == TC_ERR_ARG          # in the sizes-only form too
    d_a, d_b = torch.from_numpy(a.astype(np.int64).astype(np.int32)).cuda(), torch.from_numpy(b.astype(np.int32)).cuda()
    d_out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = C.c_uint64(64)
    assert lib.tc_lz_unparse_dev(h, C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr()), len(a), C.c_void_p(d_out.data_ptr()),
                                 C.byref(nb)) == TC_ERR_ARG
    assert bool((d_out == 0xEE).all())
    with pytest.raises(Exception):
        ctx.lz_unparse(a, b)


def test_two_contexts_interleaved(ctx):
    import textcomp
    t1, t2 = R.random_text(0x7901, 500, 2), R.periodic(333, 3) + b"q" + R.random_text(0x7902, 100, 4)
    r1, r2 = _ref(t1), _ref(t2)
    with textcomp.Context(0) as other:
        assert _dbg(other, "tc_dbg_lz_set_tile", 64) == 0       # a setting of one context is not the other's
        l1 = ctx.lpf_array(t1)
        p2 = other.lz_parse(t2)
        p1 = ctx.lz_parse(t1)
        l2 = other.lpf_array(t2)
        assert ctx.lz_unparse(*p2) == t2 and other.lz_unparse(*p1) == t1
    assert np.array_equal(l1[0], r1[0]) and np.array_equal(l1[1], r1[1])
    assert np.array_equal(l2[0], r2[0]) and np.array_equal(l2[1], r2[1])
    assert np.array_equal(p1[0], r1[2]) and np.array_equal(p1[1], r1[3])
    assert np.array_equal(p2[0], r2[2]) and np.array_equal(p2[1], r2[3])
