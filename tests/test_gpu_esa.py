"""The kept enhanced suffix array (tc_esa_build and the batched queries tc_esa_lce, tc_esa_find, tc_esa_compare) against the
reference of tests/esa_ref.py (numpy suffix array, LCP array and sparse tables; tests/test_esa_ref.py holds it to loops over the
bytes).  Everything is compared exactly.  Every batch goes through the host entry of the C ABI, through ESAHandle's host methods and
through its _dev methods, on the smallest shapes at which the kernels can go wrong: texts of 0, 1 and 2 bytes, sizes on both sides
of one workgroup of rows and of a level of the fan-out-64 tree, unary, periodic and Fibonacci texts, every byte value once, batches
on both sides of one workgroup of queries, a fan-out-4 tree of eight levels, 0 to 16 mismatches, every pair and every substring of
120-byte texts, each combination of NULL outputs, the handle's own arrays against tc_lcp_array, several contexts on one handle, the
workspace reused between the build and the queries, the error protocol, and one text of 300 001 bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import esa_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG = -1
MS = (0, 1, 4, 16)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _ref(t):
    return R.Ref(t)


def _text(seed, n, sigma):
    rng = np.random.default_rng(seed)
    alpha = (np.arange(sigma) * 256 // sigma).astype(np.uint8) if sigma > 4 else np.frombuffer(b"ACGT", np.uint8)[:sigma]
    return alpha[rng.integers(0, sigma, n)].tobytes()


def _shape(name, n):
    if name == "unary":
        return b"a" * n
    if name == "period3":
        return (b"abc" * (n // 3 + 1))[:n]
    if name == "fibonacci":
        return R.fibonacci(n)
    if name == "random2":
        return _text(0xE5A2 + n, n, 2)
    if name == "random4":
        return _text(0xE5A4 + n, n, 4)
    assert name == "all256"
    return bytes(np.random.default_rng(7).permutation(256).astype(np.uint8))[:n]


SHAPES = ("unary", "period3", "fibonacci", "random2", "random4", "all256")


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


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64).astype(np.uint32).view(np.int32).copy()).cuda()


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def _same(got, want, what):
    got, want = _np(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d wrong, first [%d] = %d, want %d" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def _lce(ctx, h, ref, a, b, ms=MS, what=""):
    a, b = _u32(a), _u32(b)
    d_a, d_b = _dev(a), _dev(b)
    for m in ms:
        wl, wm = ref.lce(a, b, m)
        tag = "%s lce n=%d nq=%d m=%d" % (what, ref.n, len(a), m)
        ln, mm = np.full(len(a), 0xabababab, np.uint32), np.full(len(a), 0xabababab, np.uint32)
        assert ctx.lib.tc_esa_lce(ctx.handle, h._h, _p(a), _p(b), len(a), m, _p(ln), _p(mm)) == 0, tag
        _same(ln, wl, tag + " abi len")
        _same(mm, wm, tag + " abi mm")
        _same(h.lce(a, b, m, ctx=ctx), wl, tag + " host, no mm")
        got = h.lce(a, b, m, mm=True, ctx=ctx)
        _same(got[0], wl, tag + " host len")
        _same(got[1], wm, tag + " host mm")
        _same(h.lce_dev(d_a, d_b, m, ctx=ctx), wl, tag + " dev, no mm")
        got = h.lce_dev(d_a, d_b, m, mm=True, ctx=ctx)
        _same(got[0], wl, tag + " dev len")
        _same(got[1], wm, tag + " dev mm")


def _find(ctx, h, ref, s, l, what=""):
    s, l = _u32(s), _u32(l)
    want = ref.find(s, l)
    tag = "%s find n=%d nq=%d" % (what, ref.n, len(s))
    out = [np.full(len(s), 0xabababab, np.uint32) for _ in range(3)]
    assert ctx.lib.tc_esa_find(ctx.handle, h._h, _p(s), _p(l), len(s), *(_p(o) for o in out)) == 0, tag
    d_s, d_l = _dev(s), _dev(l)
    for k, name in enumerate(("first_row", "occ", "first_pos")):
        _same(out[k], want[k], tag + " abi " + name)
        _same(h.find(s, l, ctx=ctx)[k], want[k], tag + " host " + name)
        _same(h.find_dev(d_s, d_l, ctx=ctx)[k], want[k], tag + " dev " + name)
    for k in range(2):
        _same(h.find(s, l, first_pos=False, ctx=ctx)[k], want[k], tag + " host, no first_pos")
        _same(h.find_dev(d_s, d_l, first_pos=False, ctx=ctx)[k], want[k], tag + " dev, no first_pos")
    return want


def _compare(ctx, h, ref, a, la, b, lb, what=""):
    q = [_u32(x) for x in (a, la, b, lb)]
    wo, wc = ref.compare(*q)
    tag = "%s compare n=%d nq=%d" % (what, ref.n, len(q[0]))
    order, common = np.full(len(q[0]), 99, np.int8), np.full(len(q[0]), 0xabababab, np.uint32)
    assert ctx.lib.tc_esa_compare(ctx.handle, h._h, *(_p(x) for x in q), len(q[0]), _p(order), _p(common)) == 0, tag
    _same(order, wo, tag + " abi order")
    _same(common, wc, tag + " abi common")
    d = [_dev(x) for x in q]
    _same(h.compare(*q, ctx=ctx), wo, tag + " host order")
    _same(h.compare(*q, common=True, ctx=ctx)[1], wc, tag + " host common")
    _same(h.compare_dev(*d, ctx=ctx), wo, tag + " dev order")
    got = h.compare_dev(*d, common=True, ctx=ctx)
    _same(got[0], wo, tag + " dev order, with common")
    _same(got[1], wc, tag + " dev common")
    return wo, wc


def _sampled(t, nq, seed, period=0):
    """pairs, substrings and pairs of substrings of t: random ones and the adversarial ones"""
    n = len(t)
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n + 1, nq), rng.integers(0, n + 1, nq)
    i = rng.integers(0, n + 1, nq)
    k = np.arange(nq) % 8
    b = np.where(k == 1, n, b)                      # (i, n)
    a = np.where(k == 2, n, a)                      # (n, i); with the next line (n, n)
    b = np.where((k == 2) & (np.arange(nq) % 16 == 2), n, b)
    b = np.where(k == 3, a, b)                      # (i, i)
    if period:
        j = np.minimum(i, max(n - period, 0))
        a, b = np.where(k == 4, j, a), np.where(k == 4, np.minimum(j + period, n), b)      # (i, i + period)
        a, b = np.where(k == 5, np.minimum(j + 3 * period, n), a), np.where(k == 5, j, b)
    a, b = np.where(k == 6, 0, a), np.where(k == 7, max(n - 1, 0), b)
    s = rng.integers(0, n + 1, nq)
    short = np.minimum(n - s, rng.integers(0, 14, nq))
    l = np.where(k < 3, rng.integers(0, n + 1, nq) % (n - s + 1), short)
    l = np.where(k == 3, 0, l)
    l = np.where(k == 4, n - s, l)                  # to the text's end: it occurs once
    s[0], l[0] = 0, n                               # len = n
    if nq > 1:
        s[1], l[1] = n, 0                           # len = 0 at position n
    s2 = rng.integers(0, n + 1, nq)
    l2 = np.where(k % 2 == 0, np.minimum(n - s2, l), rng.integers(0, n + 1, nq) % (n - s2 + 1))
    s2, l2 = np.where(k == 5, s, s2), np.where(k == 5, l // 2, l2)                            # a proper prefix
    if period:
        ok = (k == 6) & (s + period + l <= n)
        s2, l2 = np.where(ok, s + period, s2), np.where(ok, l, l2)                            # equal, at another place
    l2 = np.where(k == 7, 0, l2)
    return (a, b), (s, l), (s, l, s2, l2)


def _all_queries(ctx, h, t, nq, seed, period=0, ms=MS, what=""):
    ref = _ref(t)
    pairs, subs, quads = _sampled(t, nq, seed, period)
    _lce(ctx, h, ref, *pairs, ms=ms, what=what)
    _find(ctx, h, ref, *subs, what=what)
    _compare(ctx, h, ref, *quads, what=what)


# ------------------------------------------------------------------------------------------------ the cases
def test_tiny_texts_and_the_worked_examples(ctx):
    for t in (b"", b"a", b"ab", b"aa", b"ba"):
        with ctx.esa_build(t) as h:
            n = len(t)
            assert h.n == n
            ref = _ref(t)
            _same(h.read("sa"), ref.sa.astype(np.uint32), "sa")
            _same(h.read("lcp"), ref.lcp.astype(np.uint32), "lcp")
            _same(h.read("isa"), ref.isa.astype(np.uint32), "isa")
            assert h.read("text").tobytes() == t
            pos = np.arange(n + 1)
            a, b = np.repeat(pos, n + 1), np.tile(pos, n + 1)
            _lce(ctx, h, ref, a, b, ms=(0, 1, 16))
            subs = [(s, l) for s in range(n + 1) for l in range(n - s + 1)]
            s, l = np.array([x[0] for x in subs]), np.array([x[1] for x in subs])
            _find(ctx, h, ref, s, l)
            k = len(subs)
            _compare(ctx, h, ref, np.repeat(s, k), np.repeat(l, k), np.tile(s, k), np.tile(l, k))
    with ctx.esa_build(b"mississippi") as h:
        assert [tuple(int(x[0]) for x in h.lce([1], [4], m, mm=True)) for m in (0, 1, 2)] == [(4, 0), (5, 1), (7, 2)]
        assert h.lce([0, 3], [0, 11]).tolist() == [11, 0]
        assert [x.tolist() for x in h.find([1, 2, 0], [4, 1, 0])] == [[3, 8, 0], [2, 4, 12], [1, 2, 0]]
        order, common = h.compare([1, 1, 8], [4, 4, 2], [4, 4, 5], [4, 3, 2], common=True)
        assert order.tolist() == [0, 1, -1] and common.tolist() == [4, 3, 0] and order.dtype == np.int8


@pytest.mark.parametrize("shape", SHAPES)
def test_every_pair_and_every_substring_of_a_short_text(ctx, shape):
    t = _shape(shape, 120)
    n = len(t)
    ref = _ref(t)
    with ctx.esa_build(t) as h:
        pos = np.arange(n + 1)
        _lce(ctx, h, ref, np.repeat(pos, n + 1), np.tile(pos, n + 1), what=shape)
        s = np.concatenate([np.full(n - i + 1, i) for i in range(n + 1)])
        l = np.concatenate([np.arange(n - i + 1) for i in range(n + 1)])
        row, occ, pos1 = _find(ctx, h, ref, s, l, what=shape)
        if shape != "unary":
            assert ((occ == 1) & (l > 0) & (l < n)).any()      # substrings that occur once are among them
        rng = np.random.default_rng(120)
        i, j = rng.integers(0, len(s), 6000), rng.integers(0, len(s), 6000)
        _compare(ctx, h, ref, s[i], l[i], s[j], l[j], what=shape)
        # equal substrings at different places, proper prefixes, len 0
        eq = np.nonzero((occ >= 2) & (l > 0))[0][:2000]
        if len(eq):
            other = ref.sa[row[eq].astype(np.int64) + 1]        # another occurrence of the same substring
            other = np.where(other == s[eq], ref.sa[row[eq].astype(np.int64)], other)
            wo, wc = _compare(ctx, h, ref, s[eq], l[eq], other, l[eq], what=shape + " equal")
            assert (wo == 0).all() and (wc == l[eq]).all() and (other != s[eq]).all()
        wo, _ = _compare(ctx, h, ref, s[i], l[i], s[i], l[i] // 2, what=shape + " prefix")
        assert ((wo == 1) == (l[i] > 0)).all()
        wo, wc = _compare(ctx, h, ref, s[i], np.zeros(len(i)), s[j], l[j], what=shape + " len 0")
        assert ((wo == -1) == (l[j] > 0)).all() and (wc == 0).all()


@pytest.mark.parametrize("n", (255, 256, 257, 4095, 4096, 4097))
def test_text_sizes_around_a_workgroup_and_a_tree_level(ctx, n):
    for shape in ("unary", "period3", "random2") if n < 4095 else ("fibonacci", "random4", "unary"):
        t = _shape(shape, n)
        with ctx.esa_build(t) as h:
            _all_queries(ctx, h, t, 700, n, period={"unary": 1, "period3": 3}.get(shape, 0), what=shape)
    t = _shape("all256", 256)
    with ctx.esa_build(t) as h:
        _all_queries(ctx, h, t, 700, 256, what="all256")


@pytest.mark.parametrize("nq", (1, 255, 256, 257, 5000))
def test_batch_sizes_around_a_workgroup(ctx, nq):
    t = _text(0xBA7C, 1500, 2) + b"ab" * 300 + b"a" * 200
    with ctx.esa_build(t) as h:
        _all_queries(ctx, h, t, nq, nq, ms=(0, 4), what="batch")
        # nq = 0: TC_OK with nothing touched, whatever the pointers
        assert ctx.lib.tc_esa_lce(ctx.handle, h._h, None, None, 0, 0, None, None) == 0
        assert ctx.lib.tc_esa_find_dev(ctx.handle, h._h, None, None, 0, None, None, None) == 0
        assert ctx.lib.tc_esa_compare(ctx.handle, h._h, None, None, None, None, 0, None, None) == 0
        assert len(h.lce([], [])) == 0 and len(h.find([], [])[1]) == 0 and len(h.compare([], [], [], [])) == 0


def test_fan_out_4_tree_of_eight_levels(ctx):
    t = _text(0xF4, 20000, 4) + (b"abc" * 7000)[:20000] + b"a" * 25537
    assert len(t) == 65537
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        h = ctx.esa_build(t)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0
    with h:
        big = ctx.esa_build(t[:5000])               # fan-out 64 again: the handle keeps the fan-out it was built with
        assert h.device_bytes(5) > 8 * big.device_bytes(5)
        big.close()
        assert h.device_bytes(5) == h.device_bytes(4) - h.device_bytes(2)
        _all_queries(ctx, h, t, 3000, 4, what="fan-out 4")
        ref = _ref(t)
        rng = np.random.default_rng(44)
        i = rng.integers(40000, 65537, 1500)        # inside the unary stretch: rows far apart, long extensions
        _lce(ctx, h, ref, i, rng.integers(40000, 65537, 1500), what="fan-out 4 unary")
        _lce(ctx, h, ref, rng.integers(20000, 40000, 1500), rng.integers(20000, 39990, 1500) // 3 * 3, what="fan-out 4 period")
        _find(ctx, h, ref, i, np.minimum(65537 - i, rng.integers(1, 30, 1500)), what="fan-out 4 wide intervals")


def test_find_with_each_combination_of_null_outputs(ctx):
    import torch
    t = _shape("fibonacci", 700)
    ref = _ref(t)
    _, (s, l), _ = _sampled(t, 600, 9)
    s, l = _u32(s), _u32(l)
    want = ref.find(s, l)
    d_s, d_l = _dev(s), _dev(l)
    with ctx.esa_build(t) as h:
        for mask in range(1, 8):
            out = [np.full(len(s), 0xabababab, np.uint32) for _ in range(3)]
            assert ctx.lib.tc_esa_find(ctx.handle, h._h, _p(s), _p(l), len(s), *(_p(o) if mask >> k & 1 else None for k, o in enumerate(out))) == 0
            d_out = [torch.full((len(s),), 0x2b2b2b2b, dtype=torch.int32).cuda() for _ in range(3)]
            torch.cuda.synchronize()
            assert ctx.lib.tc_esa_find_dev(ctx.handle, h._h, C.c_void_p(d_s.data_ptr()), C.c_void_p(d_l.data_ptr()), len(s),
                                           *(C.c_void_p(o.data_ptr()) if mask >> k & 1 else None for k, o in enumerate(d_out))) == 0
            for k in range(3):
                if mask >> k & 1:
                    _same(out[k], want[k], "host mask %d output %d" % (mask, k))
                    _same(d_out[k], want[k], "dev mask %d output %d" % (mask, k))
                else:
                    assert (out[k] == 0xabababab).all() and (_np(d_out[k]) == 0x2b2b2b2b).all()


def test_arrays_are_the_librarys_own_and_serve_the_kmers(ctx):
    import torch
    t = _text(0xA77, 3000, 4) + b"acgt" * 200
    n = len(t)
    sa, lcp = ctx.lcp_array(t)
    isa = np.empty(n + 1, np.uint32)
    isa[sa] = np.arange(n + 1, dtype=np.uint32)
    with ctx.esa_build(t) as h, ctx.esa_build_dev(torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()) as hd:
        for x in (h, hd):
            assert x.n == n and x.read("text").tobytes() == t
            _same(x.read("sa"), sa, "sa")
            _same(x.read("lcp"), lcp, "lcp")
            _same(x.read("isa"), isa, "isa")
            _same(x.read_dev("sa"), sa, "sa, dev")
            _same(x.read_dev("isa", 5, 100), isa[5:105], "isa range, dev")
            _same(x.read("lcp", n, 1), lcp[n:], "the last entry")
            assert len(x.read("sa", n + 1, 0)) == 0 and x.read_dev("text", 10, 7).cpu().numpy().tobytes() == t[10:17]
            for what, first, count in (("sa", 0, n + 2), ("sa", n + 2, 0), ("text", n, 1), ("lcp", 1, 2 ** 64 - 1), (5, 0, 1), (0, 0, 1)):
                w = what if isinstance(what, int) else x.WHAT[what]
                buf = np.zeros(8, np.uint32)
                assert ctx.lib.tc_esa_read(ctx.handle, x._h, w, first, count, _p(buf), 0) == TC_ERR_ARG, (what, first, count)
        d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
        for got, want in zip(h.kmers(5, 2), ctx.kmers_dev(d_text, 5, 2)):
            _same(got, _np(want), "kmers")
        hist, distinct, total = hd.kmer_spectrum(5, 16)
        whist, wd, wt = ctx.kmer_spectrum(t, 5, 16)
        assert (distinct, total) == (wd, wt) and hist.cpu().numpy().astype(np.uint64).tolist() == whist.tolist()
        d, u = h.kmer_profile(12)
        wd, wu = ctx.kmer_profile(t, 12)
        assert d.tolist() == wd.tolist() and u.tolist() == wu.tolist()


def test_handle_outlives_the_workspace_and_serves_several_contexts(ctx):
    import textcomp
    t1, t2 = _text(1, 5000, 4) + b"ab" * 500, _shape("fibonacci", 3000)
    h1, h2 = ctx.esa_build(t1), ctx.esa_build(t2)              # two handles alive at once
    try:
        for h in (h1, h2):
            parts = [h.device_bytes(p) for p in range(6)]
            assert parts[0] == sum(parts[1:]) and all(p > 0 for p in parts)
            assert parts[1] >= h.n + 16 and parts[2] == parts[3] >= 4 * (h.n + 1) and parts[4] == parts[2] + parts[5]
            assert 13 * h.n < parts[0] < 13.3 * h.n + 1024
            assert h.device_bytes(6) == 0 and h.device_bytes(-1) == 0
        _all_queries(ctx, h1, t1, 500, 1, period=2)
        blk = ctx.encode(_text(2, 40000, 4))                    # the workspace is reused and grows: the handles are not in it
        assert ctx.decode(blk) == _text(2, 40000, 4)
        ctx.repeats(_text(3, 30000, 2), 8)
        _all_queries(ctx, h1, t1, 500, 2, period=2)
        _all_queries(ctx, h2, t2, 500, 3)
        with textcomp.Context(0) as other:                      # another context on the handle's device queries it
            _all_queries(other, h1, t1, 500, 4)
            _all_queries(ctx, h1, t1, 300, 5)
            _all_queries(other, h2, t2, 300, 6)
        _all_queries(ctx, h2, t2, 300, 7)
    finally:
        h1.close()
        h2.close()
    h1.close()                                                  # closing twice is harmless


def test_errors_leave_the_handle_and_the_context_usable(ctx):
    import torch
    t = _text(0xE44, 999, 4)
    n = len(t)
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build(t) as h:
        good = np.zeros(4, np.uint32)
        out = [np.zeros(4, np.uint32) for _ in range(3)]
        order = np.zeros(4, np.int8)

        def still_answers():
            _all_queries(ctx, h, t, 64, 3, ms=(0, 2))

        def dev(a):
            return C.c_void_p(_dev(a).data_ptr())

        # a query that leaves the text, in both forms
        for bad_a, bad_b in (([0, n + 1, 0, 0], [0, 0, 0, 0]), ([0, 0, 0, 0], [0, 0, 0xffffffff, 0])):
            a, b = _u32(bad_a), _u32(bad_b)
            assert lib.tc_esa_lce(cx, h._h, _p(a), _p(b), 4, 0, _p(out[0]), None) == TC_ERR_ARG
            d_a, d_b, d_o = _dev(a), _dev(b), _dev(good)
            torch.cuda.synchronize()
            assert lib.tc_esa_lce_dev(cx, h._h, C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr()), 4, 1, C.c_void_p(d_o.data_ptr()), None) == TC_ERR_ARG
            assert "leaves the text" in ctx.lib.tc_last_error(cx).decode()
            still_answers()
        for s, l in (([0, 0, n + 1, 0], [0, 0, 0, 0]), ([0, 0, 0, 0], [0, n + 1, 0, 0]), ([0, n, 0, 0], [0, 1, 0, 0]), ([5, 0, 0, 0], [0xfffffffe, 0, 0, 0])):
            s, l = _u32(s), _u32(l)
            assert lib.tc_esa_find(cx, h._h, _p(s), _p(l), 4, _p(out[0]), _p(out[1]), _p(out[2])) == TC_ERR_ARG
            d_s, d_l, d_o = _dev(s), _dev(l), _dev(good)
            torch.cuda.synchronize()
            assert lib.tc_esa_find_dev(cx, h._h, C.c_void_p(d_s.data_ptr()), C.c_void_p(d_l.data_ptr()), 4, None, C.c_void_p(d_o.data_ptr()), None) == TC_ERR_ARG
        still_answers()
        for k in range(4):
            q = [np.zeros(4, np.uint32) for _ in range(4)]
            q[k][2] = n + 1
            assert lib.tc_esa_compare(cx, h._h, *(_p(x) for x in q), 4, _p(order), None) == TC_ERR_ARG
            d = [_dev(x) for x in q]
            d_o = torch.zeros(4, dtype=torch.int8).cuda()
            torch.cuda.synchronize()
            assert lib.tc_esa_compare_dev(cx, h._h, *(C.c_void_p(x.data_ptr()) for x in d), 4, C.c_void_p(d_o.data_ptr()), None) == TC_ERR_ARG
        q = [_u32([0, n - 1, 0, 0]), _u32([0, 2, 0, 0]), good, good]
        assert lib.tc_esa_compare(cx, h._h, *(_p(x) for x in q), 4, _p(order), None) == TC_ERR_ARG
        still_answers()
        with pytest.raises(ctx_error()):
            h.lce([n + 1], [0])
        with pytest.raises(ctx_error()):
            h.find_dev(_dev([n]), _dev([1]))
        # nulls, too many mismatches, all three outputs of find null
        assert lib.tc_esa_lce(cx, None, _p(good), _p(good), 4, 0, _p(out[0]), None) == TC_ERR_ARG
        assert lib.tc_esa_lce(cx, h._h, None, _p(good), 4, 0, _p(out[0]), None) == TC_ERR_ARG
        assert lib.tc_esa_lce(cx, h._h, _p(good), None, 4, 0, _p(out[0]), None) == TC_ERR_ARG
        assert lib.tc_esa_lce(cx, h._h, _p(good), _p(good), 4, 0, None, _p(out[1])) == TC_ERR_ARG
        assert lib.tc_esa_lce(cx, h._h, _p(good), _p(good), 4, 17, _p(out[0]), None) == TC_ERR_ARG
        assert lib.tc_esa_lce_dev(cx, h._h, dev(good), dev(good), 4, 17, dev(good), None) == TC_ERR_ARG
        assert lib.tc_esa_lce(cx, h._h, _p(good), _p(good), 4, 16, _p(out[0]), None) == 0
        assert lib.tc_esa_find(cx, None, _p(good), _p(good), 4, _p(out[0]), None, None) == TC_ERR_ARG
        assert lib.tc_esa_find(cx, h._h, None, _p(good), 4, _p(out[0]), None, None) == TC_ERR_ARG
        assert lib.tc_esa_find(cx, h._h, _p(good), None, 4, _p(out[0]), None, None) == TC_ERR_ARG
        assert lib.tc_esa_find(cx, h._h, _p(good), _p(good), 4, None, None, None) == TC_ERR_ARG
        assert lib.tc_esa_find_dev(cx, h._h, dev(good), dev(good), 4, None, None, None) == TC_ERR_ARG
        assert lib.tc_esa_compare(cx, None, _p(good), _p(good), _p(good), _p(good), 4, _p(order), None) == TC_ERR_ARG
        assert lib.tc_esa_compare(cx, h._h, _p(good), _p(good), _p(good), _p(good), 4, None, _p(out[0])) == TC_ERR_ARG
        for k in range(4):
            q = [_p(good)] * 4
            q[k] = None
            assert lib.tc_esa_compare(cx, h._h, *q, 4, _p(order), None) == TC_ERR_ARG
        assert lib.tc_esa_read(cx, None, 2, 0, 1, _p(good), 0) == TC_ERR_ARG
        assert lib.tc_esa_read(cx, h._h, 2, 0, 1, None, 0) == TC_ERR_ARG
        hh = C.c_void_p(1)
        assert lib.tc_esa_build(cx, None, 5, C.byref(hh)) == TC_ERR_ARG and hh.value is None
        hh = C.c_void_p(1)
        assert lib.tc_esa_build_dev(cx, None, 0x7ffffff1, C.byref(hh)) == TC_ERR_ARG and hh.value is None
        assert lib.tc_esa_build(cx, None, 0, None) == TC_ERR_ARG
        assert lib.tc_esa_arrays(None, None, None, None, None) == TC_ERR_ARG and lib.tc_esa_arrays(h._h, None, None, None, None) == 0
        still_answers()
        if torch.cuda.device_count() > 1:           # a handle built on another device than the context's
            import textcomp
            with textcomp.Context(1) as far:
                assert far.lib.tc_esa_lce(far.handle, h._h, _p(good), _p(good), 4, 0, _p(out[0]), None) == TC_ERR_ARG
                assert far.lib.tc_esa_read(far.handle, h._h, 2, 0, 1, _p(good), 0) == TC_ERR_ARG
            still_answers()


def ctx_error():
    import textcomp
    return textcomp.TcError


def test_one_larger_text(ctx):
    t = _text(0x300, 200000, 4) + _text(0x301, 50000, 4) * 2 + b"a" * 1
    assert len(t) == 300001
    with ctx.esa_build(t) as h:
        ref = _ref(t)
        _same(h.read("sa"), ref.sa.astype(np.uint32), "sa")
        _same(h.read("lcp"), ref.lcp.astype(np.uint32), "lcp")
        _all_queries(ctx, h, t, 20000, 0x300, period=50000, what="300 001 bytes")
