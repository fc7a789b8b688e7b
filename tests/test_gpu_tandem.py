"""The runs (tandem repeats) of a text (tc_tandem_repeats and tc_tandem_repeats_dev) against the shift reference of
tests/tr_ref.py (tests/test_tr_ref.py holds it to the definition taken literally).  Everything is compared exactly -- the three
arrays in (start, period) order and the count -- through the host entry, the _dev entry and the sizes-only form, on the
smallest shapes at which the kernels can go wrong: text lengths on both sides of a group of the min trees at the default
fan-out and at fan-out 4, unary and two-letter periodic texts, one long run whose ends lie inside tiles, Fibonacci strings (up
to eleven runs at one start), planted tandem arrays in random DNA, runs that touch either end of the text, runs found with
exactly period - 1 bytes to the left of their root, one text of three tree levels, and the filter / capacity / sizes-only /
error protocol."""
import ctypes as C

import numpy as np
import pytest

import tr_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
SIZES = (1, 2, 3, 63, 64, 65, 4095, 4096, 4097)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(t, **f):
    """(start, len, period) of a text under filters, computed once"""
    key = (bytes(t), tuple(sorted(f.items())))
    if key not in _REF:
        _REF[key] = R.runs(t, **f)
    return _REF[key]


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _np32(t):
    return t.cpu().numpy().astype(np.uint32)


def _same(got, want, what):
    for name, g, w in zip(("start", "len", "period"), got, want):
        assert g.dtype == np.uint32 and len(g) == len(w), (what, name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s[%d] = %d, want %d" % (what, name, bad[0], g[bad[0]], w[bad[0]])


def _every_way(ctx, t, what="", **f):
    """the sizes-only form, the host entry and the _dev entry"""
    import torch
    t = bytes(t)
    want = _ref(t, **f)
    tag = "%s n=%d %r" % (what, len(t), f)
    assert ctx.tandem_repeat_count(t, **f) == len(want[0]), tag
    _same(ctx.tandem_repeats(t, **f), want, tag + " host")
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    _same(tuple(_np32(x) for x in ctx.tandem_repeats_dev(d_text, **f)), want, tag + " dev")
    return want


def _dna(seed, n):
    return np.random.RandomState(seed).randint(0, 4, n).astype(np.uint8).choose(np.frombuffer(b"ACGT", np.uint8)).tobytes()


def _planted(seed, n, units=(1, 2, 3, 5, 7, 13, 40)):
    """iid ACGT with tandem arrays written over it: one at position 0, one that ends at n - 1, the rest anywhere (a last
    copy may be cut short)"""
    rng = np.random.RandomState(seed)
    t = bytearray(_dna(seed + 1, n))
    spots = [0, None] + [int(x) for x in rng.randint(0, max(n, 1), 2 * len(units))]
    for k, at in enumerate(spots):
        p = units[k % len(units)]
        arr = (_dna(seed + 2 + k, p) * 6)[:int(rng.randint(2 * p, 5 * p + 2))][:n]
        if at is None:
            at = n - len(arr)
        at = min(at, n - len(arr))
        t[at:at + len(arr)] = arr
    return bytes(t)


def _texts(n):
    yield "unary", b"a" * n
    yield "(ab)^k", (b"ab" * n)[:n - (n & 1)] or b"a"
    yield "(ab)^k a", (b"ab" * n)[:n - 1 + (n & 1)] or b"a"
    yield "planted", _planted(0x7d00 + n, n)


# ------------------------------------------------------------------------------------------------ texts
def test_tiny_texts_and_worked_examples(ctx):
    for t in (b"", b"a", b"aa", b"ab", b"aab", b"aaa"):
        _every_way(ctx, t, repr(t))
    assert ctx.tandem_repeat_count(b"") == 0 and all(len(x) == 0 for x in ctx.tandem_repeats(b""))
    assert R.as_triples(*ctx.tandem_repeats(b"mississippi")) == [(1, 7, 3), (2, 3, 1), (5, 6, 1), (8, 9, 1)]
    assert R.as_triples(*ctx.tandem_repeats(b"aabaabaab")) == [(0, 1, 1), (0, 8, 3), (3, 4, 1), (6, 7, 1)]
    for n in (2, 3, 70):
        assert R.as_triples(*ctx.tandem_repeats(b"a" * n)) == [(0, n - 1, 1)]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_tree_groups(ctx, n):
    """n and N = n + 1 on both sides of a group of the default fan-out (64) and of a second-level group (4096)"""
    for what, t in _texts(n):
        _every_way(ctx, t, what)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_fanout_4_and_back(ctx, n):
    """trees of up to seven levels over the same texts, then the default again: the setting is per call, nothing sticks"""
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        for what, t in _texts(n):
            _every_way(ctx, t, what + ", fan-out 4")
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0
    for what, t in _texts(n):
        _every_way(ctx, t, what + ", fan-out 64 again")


def test_one_long_run_inside_tiles(ctx):
    """a random block of 4096 bytes two and a half times, between other bytes: one run of period 4096 over 10240 bytes
    whose start and end are inside tiles"""
    block = np.random.RandomState(0x7e01).randint(0, 256, 4096).astype(np.uint8).tobytes()
    t = _dna(0x7e02, 1000) + (block * 3)[:10240] + _dna(0x7e03, 700)
    s, l, p = _every_way(ctx, t, "period 4096")
    k = int(np.nonzero(p == 4096)[0][0])
    assert 0 <= 1000 - int(s[k]) < 8 and 10240 <= int(l[k]) < 10248        # (the neighbours may extend it by a byte or two)


@pytest.mark.parametrize("k", [16, 21])
def test_fibonacci_strings(ctx, k):
    """987 and 10 946 bytes: 2 F(k-2) - 3 runs, eleven of them at one start in the shorter one"""
    t = R.fibonacci(k)
    fib = [0, 1, 1]
    while len(fib) <= k:
        fib.append(fib[-1] + fib[-2])
    assert len(t) == fib[k] and len(t) in (987, 10946)
    s, _, _ = _every_way(ctx, t, "fibonacci")
    assert len(s) == 2 * fib[k - 2] - 3
    assert np.bincount(s).max() >= 11


def test_runs_at_both_ends_and_roots_with_period_minus_one_to_the_left(ctx):
    """every rotation of a unit whose Lyndon rotation (under either order) starts at its last byte, three times over, with
    nothing, a smaller and a larger byte on either side: runs that touch position 0 and position n - 1, and candidates whose
    left extension is exactly period - 1"""
    for unit in (b"abbb", b"aaab", b"mmkml"):
        for r in range(len(unit)):
            u = unit[r:] + unit[:r]
            for head in (b"", b"z"):
                for tail in (b"", b"a", b"z", u[:2]):
                    t = head + u * 3 + tail
                    want = _every_way(ctx, t, repr(t))
                    assert len(unit) in want[2].tolist()
    t = b"bbba" * 3
    assert R.as_triples(*ctx.tandem_repeats(t, min_period=2)) == [(0, len(t) - 1, 4)]


def test_three_tree_levels(ctx):
    """270 001 bytes: N above 64^3, so the searches and the range minima have a third level to climb to"""
    n = 270001
    t = _planted(0x7f00, n, units=(1, 2, 3, 5, 7, 13, 40, 64))
    want = _every_way(ctx, t, "three levels", max_period=64)
    assert len(want[0]) > 1000 and int(want[2].max()) == 64
    _every_way(ctx, b"a" * n, "three levels, unary", max_period=64)


def test_each_filter_cuts_some_runs_but_not_all(ctx):
    t = _planted(0x7f10, 3000)
    full = _every_way(ctx, t, "filters")
    z = len(full[0])
    for f in (dict(min_period=2), dict(min_period=5), dict(max_period=1), dict(max_period=7), dict(min_copies=3), dict(min_copies=4),
              dict(min_len=6), dict(min_len=40), dict(min_period=2, max_period=13, min_copies=3, min_len=10),
              dict(min_period=3, max_period=3), dict(min_len=0xffffffff), dict(min_copies=0xffffffff),
              dict(min_period=0xffffffff), dict(max_period=0xffffffff)):
        got = _every_way(ctx, t, "filters", **f)
        keep = np.array([R.passes(int(l), int(p), **f) for l, p in zip(full[1], full[2])])
        assert all(np.array_equal(g, w[keep]) for g, w in zip(got, full))
        if max(f.values()) < 0xffffffff:
            assert 0 < len(got[0]) < z, f


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _call(lib, name, h, text, n, f, start, ln, period, nrun):
    return getattr(lib, name)(h, text, n, f[0], f[1], f[2], f[3], start, ln, period, C.byref(nrun) if nrun is not None else None)


def test_capacity_and_sizes_only_host(ctx):
    lib, h = ctx.lib, ctx.handle
    t = _planted(0x7f20, 500)
    tb = np.frombuffer(t, np.uint8)
    want = _ref(t)
    z = len(want[0])
    assert z >= 2
    f = (1, 0, 2, 1)
    nrun = C.c_uint64(0)                            # sizes only
    assert _call(lib, "tc_tandem_repeats", h, _p(tb), len(tb), f, None, None, None, nrun) == 0 and nrun.value == z
    a, b, c = (np.full(len(tb), 0xDEADBEEF, np.uint32) for _ in range(3))
    nrun = C.c_uint64(z - 1)                        # one too small: the count, nothing written
    assert _call(lib, "tc_tandem_repeats", h, _p(tb), len(tb), f, _p(a), _p(b), _p(c), nrun) == TC_ERR_CAPACITY
    assert nrun.value == z and all((x == 0xDEADBEEF).all() for x in (a, b, c))
    nrun = C.c_uint64(z)                            # exact
    assert _call(lib, "tc_tandem_repeats", h, _p(tb), len(tb), f, _p(a), _p(b), _p(c), nrun) == 0 and nrun.value == z
    assert all(np.array_equal(x[:z], w) and (x[z:] == 0xDEADBEEF).all() for x, w in zip((a, b, c), want))
    nrun = C.c_uint64(len(tb))                      # capacity n is always enough
    assert _call(lib, "tc_tandem_repeats", h, _p(tb), len(tb), f, _p(a), _p(b), _p(c), nrun) == 0 and nrun.value == z


def test_capacity_and_sizes_only_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = _planted(0x7f21, 500)
    want = _ref(t)
    z = len(want[0])
    assert z >= 2
    f = (1, 0, 2, 1)
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    a, b, c = (torch.full((z + 3,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    pt, pa, pb, pc = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b, c))
    nrun = C.c_uint64(0)
    assert _call(lib, "tc_tandem_repeats_dev", h, pt, len(t), f, None, None, None, nrun) == 0 and nrun.value == z
    nrun = C.c_uint64(z - 1)
    assert _call(lib, "tc_tandem_repeats_dev", h, pt, len(t), f, pa, pb, pc, nrun) == TC_ERR_CAPACITY and nrun.value == z
    assert all(bool((x == -1).all()) for x in (a, b, c))
    nrun = C.c_uint64(z + 3)
    assert _call(lib, "tc_tandem_repeats_dev", h, pt, len(t), f, pa, pb, pc, nrun) == 0 and nrun.value == z
    assert all(np.array_equal(_np32(x[:z]), w) and bool((x[z:] == -1).all()) for x, w in zip((a, b, c), want))
    res = ctx.tandem_repeats_dev(d_text, cap=1)     # the retry loop: a first capacity that is too small
    assert all(np.array_equal(_np32(x), w) for x, w in zip(res, want))


def test_bad_arguments_and_edges(ctx):
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabraabracadabra", np.uint8)
    n = len(tb)
    a, b, c = (np.full(n, 0xDEADBEEF, np.uint32) for _ in range(3))

    def call(name="tc_tandem_repeats", text=_p(tb), n=n, min_period=1, max_period=0, min_copies=2, min_len=1, start=_p(a), ln=_p(b),
             period=_p(c), cap=n):
        nrun = C.c_uint64(cap) if cap is not None else None
        return _call(lib, name, h, text, n, (min_period, max_period, min_copies, min_len), start, ln, period, nrun), nrun

    for name in ("tc_tandem_repeats", "tc_tandem_repeats_dev"):     # (every one of these is refused before a buffer is touched)
        assert call(name, min_period=0)[0] == TC_ERR_ARG
        assert call(name, min_period=3, max_period=2)[0] == TC_ERR_ARG
        assert call(name, min_copies=1)[0] == TC_ERR_ARG and call(name, min_copies=0)[0] == TC_ERR_ARG
        assert call(name, min_len=0)[0] == TC_ERR_ARG
        assert call(name, text=None)[0] == TC_ERR_ARG
        assert call(name, n=TC_MAX_N + 1)[0] == TC_ERR_ARG
        assert call(name, cap=None)[0] == TC_ERR_ARG
        assert call(name, start=None)[0] == TC_ERR_ARG and call(name, ln=None)[0] == TC_ERR_ARG and call(name, period=None)[0] == TC_ERR_ARG
        assert call(name, start=None, ln=None, period=None)[0] == TC_ERR_ARG        # a capacity without buffers
        assert call(name, min_len=0, start=None, ln=None, period=None, cap=0)[0] == TC_ERR_ARG      # in the sizes-only form too
        rc, nrun = call(name, text=None, n=0)       # n = 0: nothing read, no runs
        assert rc == 0 and nrun.value == 0
    assert all((x == 0xDEADBEEF).all() for x in (a, b, c))
    assert call(min_period=3, max_period=3)[0] == 0
    rc, nrun = call()
    assert rc == 0 and nrun.value == len(_ref(tb.tobytes())[0]) and nrun.value >= 1
    with pytest.raises(Exception):
        ctx.tandem_repeats(b"abcabc", min_copies=1)


def test_same_answer_twice_and_from_two_contexts(ctx):
    """the order is the text's: a Fibonacci string has starts with many runs, whose slots are dealt out in arrival order
    before they are put in period order"""
    import textcomp
    t1, t2 = R.fibonacci(16) + b"q" + R.fibonacci(15), _planted(0x7f30, 2000)
    with textcomp.Context(0) as other:
        assert _dbg(other, "tc_dbg_fm_set_lcp_fanout", 4) == 0      # a setting of one context is not the other's
        a1 = ctx.tandem_repeats(t1)
        b2 = other.tandem_repeats(t2)
        b1 = other.tandem_repeats(t1)
        a2 = ctx.tandem_repeats(t2)
        again = ctx.tandem_repeats(t1)
        c1 = ctx.tandem_repeat_count(t1, min_period=3)
        c2 = other.tandem_repeat_count(t2, min_period=3)
    for got, t, what in ((a1, t1, "ctx"), (again, t1, "ctx again"), (b1, t1, "other"), (a2, t2, "ctx"), (b2, t2, "other")):
        _same(got, _ref(t), what)
    assert c1 == len(_ref(t1, min_period=3)[0]) and c2 == len(_ref(t2, min_period=3)[0])
