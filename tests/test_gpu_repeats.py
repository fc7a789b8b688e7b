"""The maximal and supermaximal repeats of a text (tc_repeats and tc_repeats_dev) against the reference of tests/rep_ref.py
(the suffix-array rule by a stack walk; tests/test_rep_ref.py holds it to brute force over all substrings).  Everything is
compared exactly -- the four arrays in the order of the representative rows, the count, the suffix array -- through the host
and the _dev entry and for both kinds, on the smallest shapes at which the kernels can go wrong: row counts on both sides of
a group of the min tree at the default fan-out and at fan-out 4, of a tile of the count and fill passes, unary texts around
the 257 occurrences the supermaximal kind can see, the two 257-occurrence texts, repeats that are a prefix or a suffix of the
text, and the filter / capacity / sizes-only / error protocol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rep_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "text-compression_amd", "csrc", "tc_rep.hpp")).read()
REP_TILE = int(re.search(r"#define REP_NT (\d+)", _SRC).group(1)) * int(re.search(r"#define REP_ITEMS (\d+)", _SRC).group(1))
KINDS = (R.MAXIMAL, R.SUPERMAXIMAL)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(t, kind, min_len=1, min_occ=2):
    """(pos, len, occ, row, sa) of a text, computed once"""
    key = (bytes(t), kind, min_len, min_occ)
    if key not in _REF:
        _REF[key] = R.repeats(t, kind, min_len, min_occ)
    return _REF[key]


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _np32(t):
    return t.cpu().numpy().astype(np.uint32)


def _same(got, want, what):
    for name, g, w in zip(("pos", "len", "occ", "row", "sa"), got, want):
        assert g.dtype == np.uint32 and len(g) == len(w), (what, name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s[%d] = %d, want %d" % (what, name, bad[0], g[bad[0]], w[bad[0]])


def _every_way(ctx, t, what="", min_len=1, min_occ=2):
    """both kinds, through the host and the _dev entry, the sizes-only form included"""
    import torch
    t = bytes(t)
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    for kind in KINDS:
        want = _ref(t, kind, min_len, min_occ)
        tag = "%s n=%d kind=%d min_len=%d min_occ=%d" % (what, len(t), kind, min_len, min_occ)
        assert ctx.repeat_count(t, min_len, min_occ, supermaximal=bool(kind)) == len(want[0]), tag
        _same(ctx.repeats(t, min_len, min_occ, supermaximal=bool(kind), with_sa=True), want, tag + " host")
        _same(tuple(_np32(x) for x in ctx.repeats_dev(d_text, min_len, min_occ, supermaximal=bool(kind), with_sa=True)), want,
              tag + " dev")


def _named(t, got):
    return {w.decode("latin-1"): len(ps) for w, ps in R.as_dict(t, *got).items()}


# ------------------------------------------------------------------------------------------------ texts
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"aa", b"ab"):
        _every_way(ctx, t, repr(t))
    assert ctx.repeat_count(b"") == 0
    pos, ln, occ, row, sa = ctx.repeats(b"", with_sa=True)
    assert len(pos) == len(ln) == len(occ) == len(row) == 0 and sa.tolist() == [0]
    assert _named(b"aa", ctx.repeats(b"aa", with_sa=True)) == {"a": 2}


def test_worked_examples(ctx):
    def both(t):
        _every_way(ctx, t, repr(t))
        return (_named(t, ctx.repeats(t, with_sa=True)), _named(t, ctx.repeats(t, supermaximal=True, with_sa=True)))
    assert both(b"mississippi") == ({"i": 4, "issi": 2, "p": 2, "s": 4}, {"issi": 2, "p": 2})
    assert both(b"a" * 8) == ({"a" * k: 9 - k for k in range(1, 8)}, {"a" * 7: 2})
    assert both(b"abcabcabc") == ({"abc": 3, "abcabc": 2}, {"abcabc": 2})
    pos, ln, occ, row = ctx.repeats(b"aaabaab")         # the order of the header's example: not sorted by row
    assert (row.tolist(), ln.tolist(), occ.tolist(), pos.tolist()) == ([1, 2, 1], [2, 3, 1], [3, 2, 5], [0, 4, 0])


@pytest.mark.parametrize("n", [64, 257, 258, 300])
def test_unary_around_the_supermaximal_limit(ctx, n):
    """a^k occurs n + 1 - k times: occ runs through 257 and 258, all left contexts but one equal"""
    _every_way(ctx, b"a" * n, "unary")
    _every_way(ctx, b"a" * n, "unary", min_occ=257)
    _every_way(ctx, b"a" * n, "unary", min_occ=258)


def test_structured_texts(ctx):
    for p in (2, 3, 7):
        _every_way(ctx, R.periodic(100, p), "period %d" % p)
        _every_way(ctx, R.periodic(1000, p) + b"z" + R.periodic(300, p), "period %d twice" % p)
    _every_way(ctx, R.fibonacci(200), "fibonacci")
    _every_way(ctx, R.fibonacci(3000), "fibonacci")


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 4095, 4096, 4097,
                               2 * REP_TILE - 2, 2 * REP_TILE - 1, 2 * REP_TILE, 2 * REP_TILE + 1])
def test_random_texts_at_group_and_tile_boundaries(ctx, n):
    """n and N = n + 1 on both sides of a group of the default fan-out (64), of a second-level group (4096) and of two
    tiles of the count and fill passes"""
    for sigma in (1, 2, 4, 256):
        _every_way(ctx, R.random_text(0x8100 + 7 * n + sigma, n, sigma), "random over %d" % sigma)


@pytest.mark.parametrize("n", [1024, 1025, 4096, 4097])
def test_fanout_4(ctx, n):
    """trees of 5 and 6 levels, on the texts whose nearest smaller rows are far"""
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        _every_way(ctx, b"a" * n, "unary, fan-out 4")
        for p in (2, 3, 7):
            _every_way(ctx, R.periodic(n, p), "period %d, fan-out 4" % p)
        _every_way(ctx, R.fibonacci(n), "fibonacci, fan-out 4")
        for sigma in (2, 4, 256):
            _every_way(ctx, R.random_text(0x8200 + n + sigma, n, sigma), "random over %d, fan-out 4" % sigma)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0


def test_257_distinct_left_contexts(ctx):
    """w = 01 02 03 occurs 257 times with every left context another one, Nothing among them: the most the supermaximal
    kind can see; with one left context doubled w is maximal but not supermaximal"""
    w = bytes([1, 2, 3])
    t = R.many_left()
    _every_way(ctx, t, "257 left contexts")
    sup = R.as_dict(t, *ctx.repeats(t, supermaximal=True, with_sa=True))
    assert len(sup[w]) == 257 and 0 in sup[w]
    t2 = R.many_left(doubled=7)
    _every_way(ctx, t2, "a left context twice")
    assert w not in R.as_dict(t2, *ctx.repeats(t2, supermaximal=True, with_sa=True))
    assert len(R.as_dict(t2, *ctx.repeats(t2, with_sa=True))[w]) == 257


def test_repeat_that_is_a_prefix_and_one_that_is_a_suffix(ctx):
    """the primary row inside a reported interval (Nothing is a left context like any other), and the end-of-text rule"""
    t = b"abcXabcYabc"
    _every_way(ctx, t, "prefix and suffix")
    pos, ln, occ, row, sa = ctx.repeats(t, with_sa=True)
    k = [i for i in range(len(pos)) if t[pos[i]:pos[i] + ln[i]] == b"abc"][0]
    primary = int(np.nonzero(sa == 0)[0][0])
    assert int(occ[k]) == 3 and int(row[k]) <= primary < int(row[k]) + 3
    assert len(t) - 3 in sa[row[k]:row[k] + 3].tolist()
    # all left contexts equal but for the start of the text; all right contexts equal but for its end
    assert _named(b"abXab", ctx.repeats(b"abXab", with_sa=True)) == {"ab": 2}
    assert _named(b"XabXab", ctx.repeats(b"XabXab", with_sa=True)) == {"Xab": 2}
    assert _named(b"abXabX", ctx.repeats(b"abXabX", with_sa=True)) == {"abX": 2}


def test_filters_cut_none_some_and_all(ctx):
    t = R.random_text(0x8301, 3000, 4)
    full = _ref(t, R.MAXIMAL)
    longest, most = int(full[1].max()), int(full[2].max())
    assert longest >= 8 and most > 300
    for min_len, min_occ in ((1, 2), (4, 2), (1, 5), (6, 3), (longest, 2), (longest + 1, 2), (1, most), (1, most + 1), (20, 2),
                             (0xffffffff, 2), (1, 0xffffffff)):
        _every_way(ctx, t, "filters", min_len, min_occ)
    assert len(_ref(t, R.MAXIMAL, 4, 2)[0]) < len(full[0])
    assert len(_ref(t, R.MAXIMAL, longest + 1, 2)[0]) == 0 and len(_ref(t, R.MAXIMAL, longest, 2)[0]) >= 1


def test_pos_is_sa_of_row_and_sa_is_the_suffix_array(ctx):
    t = R.fibonacci(500) + R.random_text(0x8302, 500, 2)
    for kind in KINDS:
        pos, ln, occ, row, sa = ctx.repeats(t, supermaximal=bool(kind), with_sa=True)
        assert len(pos) > 0 and np.array_equal(pos, sa[row])
        assert np.array_equal(sa, ctx.suffix_array(t))
        assert int((row.astype(np.int64) + occ).max()) <= len(t) + 1


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _call(lib, h, name, text, n, kind, min_len, min_occ, sa, pos, ln, occ, row, nrep):
    fn = getattr(lib, name)
    return fn(h, text, n, kind, min_len, min_occ, sa, pos, ln, occ, row, C.byref(nrep) if nrep is not None else None)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_sizes_only_and_null_row_and_sa_host(ctx, kind):
    lib, h = ctx.lib, ctx.handle
    t = R.random_text(0x8401, 400, 2)
    tb = np.frombuffer(t, np.uint8)
    want = _ref(t, kind)
    z = len(want[0])
    assert z >= 2
    nrep = C.c_uint64(0)                            # sizes only
    assert _call(lib, h, "tc_repeats", _p(tb), len(tb), kind, 1, 2, None, None, None, None, None, nrep) == 0 and nrep.value == z
    a, b, c, d = (np.full(z, 0xDEADBEEF, np.uint32) for _ in range(4))
    nrep = C.c_uint64(z - 1)                        # one too small: the count, nothing written
    assert _call(lib, h, "tc_repeats", _p(tb), len(tb), kind, 1, 2, None, _p(a), _p(b), _p(c), _p(d), nrep) == TC_ERR_CAPACITY
    assert nrep.value == z
    assert all((x == 0xDEADBEEF).all() for x in (a, b, c, d))
    nrep = C.c_uint64(z)                            # exact; no row, no sa
    assert _call(lib, h, "tc_repeats", _p(tb), len(tb), kind, 1, 2, None, _p(a), _p(b), _p(c), None, nrep) == 0 and nrep.value == z
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(c, want[2]) and (d == 0xDEADBEEF).all()
    sa = np.zeros(len(tb) + 1, np.uint32)
    nrep = C.c_uint64(len(tb))                      # capacity n is always enough
    assert _call(lib, h, "tc_repeats", _p(tb), len(tb), kind, 1, 2, _p(sa), _p(a), _p(b), _p(c), _p(d), nrep) == 0 and nrep.value == z
    assert np.array_equal(d, want[3]) and np.array_equal(sa, want[4])


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_sizes_only_and_null_row_and_sa_dev(ctx, kind):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = R.random_text(0x8402, 400, 2)
    want = _ref(t, kind)
    z = len(want[0])
    assert z >= 2
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    a, b, c, d = (torch.full((z,), -1, dtype=torch.int32, device="cuda") for _ in range(4))
    d_sa = torch.full((len(t) + 1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pt, pa, pb, pc, pd, ps = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b, c, d, d_sa))
    nrep = C.c_uint64(0)
    assert _call(lib, h, "tc_repeats_dev", pt, len(t), kind, 1, 2, None, None, None, None, None, nrep) == 0 and nrep.value == z
    nrep = C.c_uint64(z - 1)
    assert _call(lib, h, "tc_repeats_dev", pt, len(t), kind, 1, 2, None, pa, pb, pc, pd, nrep) == TC_ERR_CAPACITY and nrep.value == z
    assert all(bool((x == -1).all()) for x in (a, b, c, d))
    nrep = C.c_uint64(z)
    assert _call(lib, h, "tc_repeats_dev", pt, len(t), kind, 1, 2, None, pa, pb, pc, None, nrep) == 0 and nrep.value == z
    assert np.array_equal(_np32(a), want[0]) and np.array_equal(_np32(b), want[1]) and np.array_equal(_np32(c), want[2])
    assert bool((d == -1).all())
    nrep = C.c_uint64(z)
    assert _call(lib, h, "tc_repeats_dev", pt, len(t), kind, 1, 2, ps, pa, pb, pc, pd, nrep) == 0 and nrep.value == z
    assert np.array_equal(_np32(d), want[3]) and np.array_equal(_np32(d_sa), want[4])
    res = ctx.repeats_dev(d_text, supermaximal=bool(kind), cap=1)       # the retry loop: a first capacity that is too small
    assert all(np.array_equal(_np32(x), w) for x, w in zip(res, want[:4]))


def test_bad_arguments_and_edges(ctx):
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabra", np.uint8)
    n = len(tb)
    a, b, c, d = (np.full(n, 0xDEADBEEF, np.uint32) for _ in range(4))

    def call(text=_p(tb), n=n, kind=0, min_len=1, min_occ=2, sa=None, pos=_p(a), ln=_p(b), occ=_p(c), row=_p(d), cap=n):
        nrep = C.c_uint64(cap) if cap is not None else None
        return _call(lib, h, "tc_repeats", text, n, kind, min_len, min_occ, sa, pos, ln, occ, row, nrep), nrep

    assert call(min_len=0)[0] == TC_ERR_ARG                     # the four argument errors of the header
    assert call(min_occ=1)[0] == TC_ERR_ARG and call(min_occ=0)[0] == TC_ERR_ARG
    assert call(kind=2)[0] == TC_ERR_ARG and call(kind=-1)[0] == TC_ERR_ARG
    assert call(text=None)[0] == TC_ERR_ARG
    assert call(n=TC_MAX_N + 1)[0] == TC_ERR_ARG
    assert call(cap=None)[0] == TC_ERR_ARG
    assert call(pos=None)[0] == TC_ERR_ARG and call(ln=None)[0] == TC_ERR_ARG and call(occ=None)[0] == TC_ERR_ARG
    assert call(pos=None, ln=None, occ=None)[0] == TC_ERR_ARG   # a capacity without buffers
    assert call(min_len=0, pos=None, ln=None, occ=None, cap=0)[0] == TC_ERR_ARG     # in the sizes-only form too
    assert all((x == 0xDEADBEEF).all() for x in (a, b, c, d))
    sa = np.full(1, 0xDEADBEEF, np.uint32)
    rc, nrep = call(text=None, n=0, sa=_p(sa))                  # n = 0: nothing read, no repeats, the one row
    assert rc == 0 and nrep.value == 0 and sa.tolist() == [0]
    rc, nrep = call()
    assert rc == 0 and nrep.value == len(_ref(tb.tobytes(), R.MAXIMAL)[0])
    with pytest.raises(Exception):
        ctx.repeats(b"abc", min_len=0)
    import torch
    d_sa = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nrep = C.c_uint64(0)
    assert _call(lib, h, "tc_repeats_dev", None, 0, 0, 1, 2, C.c_void_p(d_sa.data_ptr()), None, None, None, None, nrep) == 0
    assert nrep.value == 0 and d_sa.cpu().tolist() == [0]


def test_two_contexts_interleaved(ctx):
    import textcomp
    t1, t2 = R.random_text(0x8501, 500, 2), R.periodic(333, 3) + b"q" + R.random_text(0x8502, 100, 4)
    with textcomp.Context(0) as other:
        assert _dbg(other, "tc_dbg_fm_set_lcp_fanout", 4) == 0      # a setting of one context is not the other's
        a1 = ctx.repeats(t1, with_sa=True)
        b2 = other.repeats(t2, supermaximal=True, with_sa=True)
        b1 = ctx.repeats(t1, supermaximal=True, with_sa=True)
        a2 = other.repeats(t2, with_sa=True)
        c1 = ctx.repeat_count(t1, min_len=3)
        c2 = other.repeat_count(t2, min_len=3)
    _same(a1, _ref(t1, R.MAXIMAL), "ctx, maximal")
    _same(b1, _ref(t1, R.SUPERMAXIMAL), "ctx, supermaximal")
    _same(a2, _ref(t2, R.MAXIMAL), "other, maximal")
    _same(b2, _ref(t2, R.SUPERMAXIMAL), "other, supermaximal")
    assert c1 == len(_ref(t1, R.MAXIMAL, 3)[0]) and c2 == len(_ref(t2, R.MAXIMAL, 3)[0])
