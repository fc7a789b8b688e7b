"""The palindromes and inverted repeats of a text (tc_palindromes, tc_longest_palindrome and their _dev forms) against the numpy
reference of tests/pal_ref.py (tests/test_pal_ref.py holds it to the definition taken literally).  Everything is compared
exactly -- the three arrays in centre order and the count -- through the sizes-only form, the host entry and the _dev entry, on
the smallest shapes at which the kernels can go wrong: text lengths that put the 2n + 1 rows of the joint text on both sides of
a first-level and a second-level group of the min tree at the default fan-out and at fan-out 4, unary texts (the clamp at nearly
every centre), two-letter periodic texts, texts that are one palindrome as a whole, planted palindromes and reverse-complement
stems with substitutions next to the centre and at the outer edge, Fibonacci strings, the budget 16, one text of three tree
levels, the byte values 0 and 255, and the min_len / capacity / sizes-only / error protocol."""
import ctypes as C

import numpy as np
import pytest

import pal_ref as R

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
SIZES = (1, 2, 3, 31, 32, 33, 2047, 2048, 2049)
SIGMAS = (("identity", None), ("complement", R.DNA))


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(t, comp=None, m=0, min_len=1):
    """(start, len, mm) of a text, computed once"""
    key = (bytes(t), None if comp is None else bytes(comp), m, min_len)
    if key not in _REF:
        _REF[key] = R.palindromes(np.frombuffer(bytes(t), np.uint8), comp, m, min_len)
    return _REF[key]


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _np32(t):
    return t.cpu().numpy().astype(np.uint32)


def _same(got, want, what):
    for name, g, w in zip(("start", "len", "mm"), got, want):
        assert g.dtype == np.uint32 and len(g) == len(w), (what, name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s[%d] = %d, want %d" % (what, name, bad[0], g[bad[0]], w[bad[0]])


def _longest_of(want):
    s, ln, mm = want
    if not len(ln):
        return 0, 0, 0
    k = int(np.argmax(ln))                          # the first of the maxima: the smallest centre
    return int(s[k]), int(ln[k]), int(mm[k])


def _every_way(ctx, t, comp=None, m=0, min_len=1, what="", longest=True):
    """the sizes-only form, the host entry and the _dev entry; and both longest calls against the list"""
    import torch
    t = bytes(t)
    want = _ref(t, comp, m, min_len)
    tag = "%s n=%d m=%d min_len=%d %s" % (what, len(t), m, min_len, "identity" if comp is None else "sigma")
    assert ctx.palindrome_count(t, comp, m, min_len) == len(want[0]), tag
    _same(ctx.palindromes(t, comp, m, min_len), want, tag + " host")
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    _same(tuple(_np32(x) for x in ctx.palindromes_dev(d_text, comp, m, min_len)), want, tag + " dev")
    if longest:
        top = _longest_of(_ref(t, comp, m, 1))
        assert ctx.longest_palindrome(t, comp, m) == top, tag + " longest"
        assert ctx.longest_palindrome_dev(d_text, comp, m) == top, tag + " longest dev"
    return want


def _texts(n, comp):
    rng = np.random.default_rng(0x9a00 + n)
    yield "unary", b"a" * n
    yield "unary N", b"N" * n
    yield "(ab)^k", (b"ab" * n)[:n]
    w = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n + 1) // 2).astype(np.uint8)
    yield "w reverse(w)", bytes(np.concatenate((w, w[::-1][n & 1:])))
    yield "w sigma(reverse(w))", bytes(np.concatenate((w, R.DNA[w[::-1]][n & 1:])))
    yield "planted", bytes(R.planted(rng, n, comp))


# ------------------------------------------------------------------------------------------------ texts
def test_tiny_texts_and_worked_examples(ctx):
    for t in (b"", b"a", b"aa", b"ab", b"aba"):
        for _, comp in SIGMAS:
            for m in (0, 1):
                _every_way(ctx, t, comp, m, what=repr(t))
    assert ctx.palindrome_count(b"") == 0 and all(len(x) == 0 for x in ctx.palindromes(b""))
    assert ctx.longest_palindrome(b"") == (0, 0, 0)
    assert R.as_triples(*ctx.palindromes(b"mississippi", min_len=3)) == [(1, 4, 0), (1, 7, 0), (4, 4, 0), (7, 4, 0)]
    assert R.as_triples(*ctx.palindromes(b"ACGT", R.DNA)) == [(0, 4, 0)]
    assert R.as_triples(*ctx.palindromes(b"ACAGT", R.DNA)) == []
    assert R.as_triples(*ctx.palindromes(b"ACAGT", R.DNA, 1)) == [(0, 5, 1), (2, 3, 1)]
    for t, m in ((b"ACGT", 0), (b"ACAGT", 0), (b"ACAGT", 1)):
        _every_way(ctx, t, R.DNA, m, what=repr(t))
    import textcomp
    assert R.as_triples(*ctx.palindromes(b"ACGT", textcomp.DNA_COMPLEMENT)) == [(0, 4, 0)]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_tree_groups(ctx, n):
    """2n + 1 rows on both sides of a group of the default fan-out (64) and of a second-level group (4096)"""
    for _, comp in SIGMAS:
        for what, t in _texts(n, comp):
            for m in (0, 1, 3):
                _every_way(ctx, t, comp, m, what=what)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_fanout_4_and_back(ctx, n):
    """trees of up to seven levels over the same texts, then the default again: the setting is per call, nothing sticks"""
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        for _, comp in SIGMAS:
            for what, t in _texts(n, comp):
                for m in (0, 1, 3):
                    _every_way(ctx, t, comp, m, what=what + ", fan-out 4")
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0
    for _, comp in SIGMAS:
        for what, t in _texts(n, comp):
            _every_way(ctx, t, comp, 1, what=what + ", fan-out 64 again")


def test_whole_text_and_planted_stems_are_found(ctx):
    """what the families are for: the whole text is one palindrome; a planted stem with substitutions is found within the budget
    and not without it; the trim decides where a mismatch lies at the outer edge"""
    n = 2048
    fam = dict(_texts(n, R.DNA))
    s, ln, mm = _every_way(ctx, fam["w reverse(w)"], None, 0, what="whole")
    assert (0, n, 0) in R.as_triples(s, ln, mm)
    s, ln, mm = _every_way(ctx, fam["w sigma(reverse(w))"], R.DNA, 0, what="whole")
    assert (0, n, 0) in R.as_triples(s, ln, mm)
    stem = b"ACGGTCATTCAGGCTA"
    arm = bytes(R.DNA[np.frombuffer(stem, np.uint8)[::-1]])
    assert arm[:1] == b"T" and arm[-1:] == b"T"
    edge = b"G" + arm[1:-1] + b"C"                  # a substitution next to the centre and one at the outer edge
    for head in (b"", b"GGAT"):
        t = head + stem + edge + b"TT"
        for m in (0, 1, 2):
            want = R.as_triples(*_every_way(ctx, t, R.DNA, m, what="stem"))
            at = [x for x in want if 2 * x[0] + x[1] - 1 == 2 * len(head) + 31]
            if m == 0:
                assert at == []
            else:                                   # (the outer pair is a mismatch: 30 bytes with one mismatch, never 32 with two)
                assert at == [(len(head) + 1, 30, 1)]


@pytest.mark.parametrize("k", [16, 21])
def test_fibonacci_strings(ctx, k):
    """987 and 10 946 bytes, palindrome-rich: every prefix ends in a long one"""
    t = R.fibonacci(k)
    assert len(t) in (987, 10946)
    for m in (0, 2):
        s, ln, _ = _every_way(ctx, t, None, m, what="fibonacci")
        assert int(ln.max()) > len(t) // 2
    _every_way(ctx, t.replace(b"a", b"A").replace(b"b", b"T"), R.DNA, 2, what="fibonacci AT")


def test_budget_16(ctx):
    rng = np.random.default_rng(0x9b00)
    for _, comp in SIGMAS:
        t = bytes(R.planted(rng, 3000, comp, count=20))
        s, ln, mm = _every_way(ctx, t, comp, 16, what="m=16")
        assert int(mm.max()) == 16 and int(mm.min()) == 0
        t = bytes(R.planted(rng, 40, comp))          # the budget exceeds every radius
        _every_way(ctx, t, comp, 16, what="m=16, 40 bytes")


def test_three_tree_levels(ctx):
    """135 001 bytes: 2n + 1 above 64^3, so the range minima have a third level to climb to"""
    n = 135001
    rng = np.random.default_rng(0x9b10)
    t = bytes(R.planted(rng, n, R.DNA, count=400))
    for m in (0, 2):
        want = _every_way(ctx, t, R.DNA, m, 8, what="three levels")
        assert len(want[0]) > 100
    want = _every_way(ctx, b"a" * n, None, 0, what="three levels, unary")
    assert len(want[0]) == 2 * n - 1 and _longest_of(want) == (0, n, 0)
    assert ctx.palindrome_count(b"A" * n, R.DNA, 2) == 0


def test_bytes_0_and_255_and_a_sigma_that_swaps_them(ctx):
    """no byte is special in the joint text"""
    swap = R.IDENTITY.copy()
    swap[0], swap[255] = 255, 0
    rng = np.random.default_rng(0x9b20)
    for n in (5, 64, 700):
        t = rng.choice(np.array([0, 255, 7], np.uint8), n).astype(np.uint8)
        half = t[:n // 2]
        for comp in (None, swap):
            _every_way(ctx, t, comp, 1, what="0/255")
            whole = np.concatenate((half, (R.IDENTITY if comp is None else swap)[half[::-1]]))
            want = _every_way(ctx, whole, comp, 0, what="0/255 whole")
            assert _longest_of(want)[1] == len(whole)
        _every_way(ctx, bytes([0]) * n, swap, 1, what="all 0")
        _every_way(ctx, bytes([255]) * n, None, 0, what="all 255")


def test_min_len_cuts_some_palindromes_but_not_all(ctx):
    rng = np.random.default_rng(0x9b30)
    for _, comp in SIGMAS:
        t = bytes(R.planted(rng, 3000, comp))
        full = _every_way(ctx, t, comp, 1, what="min_len")
        z = len(full[0])
        for min_len in (3, 6, 12, 0xffffffff):
            got = _every_way(ctx, t, comp, 1, min_len, what="min_len", longest=False)
            keep = full[1] >= min_len
            assert all(np.array_equal(g, w[keep]) for g, w in zip(got, full))
            if min_len < 0xffffffff:
                assert 0 < len(got[0]) < z, min_len
            else:
                assert len(got[0]) == 0


def test_longest_palindrome(ctx):
    import torch
    assert ctx.longest_palindrome(b"ACAC", R.DNA, 0) == (0, 0, 0)      # no fixed point, no matching pair
    d = torch.from_numpy(np.frombuffer(b"ACAC", np.uint8).copy()).cuda()
    assert ctx.longest_palindrome_dev(d, R.DNA, 0) == (0, 0, 0)
    assert ctx.longest_palindrome(b"abab") == (0, 3, 0)                # aba and bab: the smaller centre wins
    assert ctx.longest_palindrome(b"mississippi") == (1, 7, 0)
    assert ctx.longest_palindrome(b"xabcbay" * 3) == (1, 5, 0)         # three of one length: the first
    assert ctx.longest_palindrome(b"ACAGT", R.DNA, 1) == (0, 5, 1)


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _call(lib, name, h, text, n, comp, m, min_len, start, ln, mm, npal):
    return getattr(lib, name)(h, text, n, comp, m, min_len, start, ln, mm, C.byref(npal) if npal is not None else None)


def test_capacity_and_sizes_only_host(ctx):
    lib, h = ctx.lib, ctx.handle
    t = bytes(R.planted(np.random.default_rng(0x9b40), 500, R.DNA))
    tb = np.frombuffer(t, np.uint8)
    comp = _p(R.DNA)
    want = _ref(t, R.DNA, 1, 4)
    z = len(want[0])
    assert z >= 2
    npal = C.c_uint64(0)                            # sizes only
    assert _call(lib, "tc_palindromes", h, _p(tb), len(tb), comp, 1, 4, None, None, None, npal) == 0 and npal.value == z
    a, b, c = (np.full(2 * len(tb), 0xDEADBEEF, np.uint32) for _ in range(3))
    npal = C.c_uint64(z - 1)                        # one too small: the count, nothing written
    assert _call(lib, "tc_palindromes", h, _p(tb), len(tb), comp, 1, 4, _p(a), _p(b), _p(c), npal) == TC_ERR_CAPACITY
    assert npal.value == z and all((x == 0xDEADBEEF).all() for x in (a, b, c))
    npal = C.c_uint64(z)                            # exact
    assert _call(lib, "tc_palindromes", h, _p(tb), len(tb), comp, 1, 4, _p(a), _p(b), _p(c), npal) == 0 and npal.value == z
    assert all(np.array_equal(x[:z], w) and (x[z:] == 0xDEADBEEF).all() for x, w in zip((a, b, c), want))
    full = _ref(t, None, 0, 1)                      # capacity 2n - 1 is always enough (the identity: every centre of a byte reports)
    npal = C.c_uint64(2 * len(tb) - 1)
    assert _call(lib, "tc_palindromes", h, _p(tb), len(tb), None, 0, 1, _p(a), _p(b), _p(c), npal) == 0 and npal.value == len(full[0])
    assert all(np.array_equal(x[:len(w)], w) for x, w in zip((a, b, c), full))
    a[:], b[:], c[:] = 0xDEADBEEF, 0xDEADBEEF, 0xDEADBEEF       # pal_mm alone may be null: the other two as before, it untouched
    npal = C.c_uint64(z)
    assert _call(lib, "tc_palindromes", h, _p(tb), len(tb), comp, 1, 4, _p(a), _p(b), None, npal) == 0 and npal.value == z
    assert np.array_equal(a[:z], want[0]) and np.array_equal(b[:z], want[1]) and (c == 0xDEADBEEF).all()


def test_capacity_and_sizes_only_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = bytes(R.planted(np.random.default_rng(0x9b41), 500, R.DNA))
    comp = _p(R.DNA)
    want = _ref(t, R.DNA, 1, 4)
    z = len(want[0])
    assert z >= 2
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    a, b, c = (torch.full((z + 3,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    pt, pa, pb, pc = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b, c))
    npal = C.c_uint64(0)
    assert _call(lib, "tc_palindromes_dev", h, pt, len(t), comp, 1, 4, None, None, None, npal) == 0 and npal.value == z
    npal = C.c_uint64(z - 1)
    assert _call(lib, "tc_palindromes_dev", h, pt, len(t), comp, 1, 4, pa, pb, pc, npal) == TC_ERR_CAPACITY and npal.value == z
    assert all(bool((x == -1).all()) for x in (a, b, c))
    npal = C.c_uint64(z + 3)
    assert _call(lib, "tc_palindromes_dev", h, pt, len(t), comp, 1, 4, pa, pb, None, npal) == 0 and npal.value == z
    assert np.array_equal(_np32(a[:z]), want[0]) and np.array_equal(_np32(b[:z]), want[1]) and bool((c == -1).all())
    npal = C.c_uint64(z + 3)
    assert _call(lib, "tc_palindromes_dev", h, pt, len(t), comp, 1, 4, pa, pb, pc, npal) == 0 and npal.value == z
    assert all(np.array_equal(_np32(x[:z]), w) and bool((x[z:] == -1).all()) for x, w in zip((a, b, c), want))
    res = ctx.palindromes_dev(d_text, R.DNA, 1, 4, cap=1)       # the retry loop: a first capacity that is too small
    assert all(np.array_equal(_np32(x), w) for x, w in zip(res, want))


def test_bad_arguments_and_edges(ctx):
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabraabracadabra", np.uint8)
    n = len(tb)
    a, b, c = (np.full(2 * n, 0xDEADBEEF, np.uint32) for _ in range(3))
    bad = R.IDENTITY.copy()
    bad[65], bad[66] = 66, 67
    words = [C.c_uint32(0xDEADBEEF) for _ in range(3)]

    def call(name="tc_palindromes", text=_p(tb), n=n, comp=None, m=0, min_len=1, start=_p(a), ln=_p(b), mm=_p(c), cap=2 * n):
        npal = C.c_uint64(cap) if cap is not None else None
        return _call(lib, name, h, text, n, comp, m, min_len, start, ln, mm, npal), npal

    def longest(name, text=_p(tb), n=n, comp=None, m=0, out=(0, 1, 2)):
        return getattr(lib, name)(h, text, n, comp, m, *(C.byref(words[k]) if k in out else None for k in range(3)))

    for name in ("tc_palindromes", "tc_palindromes_dev"):       # (every one of these is refused before a buffer is touched)
        assert call(name, min_len=0)[0] == TC_ERR_ARG
        assert call(name, m=17)[0] == TC_ERR_ARG
        assert call(name, comp=_p(bad))[0] == TC_ERR_ARG
        assert call(name, text=None)[0] == TC_ERR_ARG
        assert call(name, n=TC_MAX_N // 2 + 1)[0] == TC_ERR_ARG
        assert call(name, cap=None)[0] == TC_ERR_ARG
        assert call(name, start=None)[0] == TC_ERR_ARG and call(name, ln=None)[0] == TC_ERR_ARG
        assert call(name, start=None, ln=None, mm=None)[0] == TC_ERR_ARG            # a capacity without buffers
        assert call(name, min_len=0, start=None, ln=None, mm=None, cap=0)[0] == TC_ERR_ARG      # in the sizes-only form too
        assert call(name, m=17, start=None, ln=None, mm=None, cap=0)[0] == TC_ERR_ARG
        rc, npal = call(name, text=None, n=0)       # n = 0: nothing read, no palindromes
        assert rc == 0 and npal.value == 0
    assert all((x == 0xDEADBEEF).all() for x in (a, b, c))
    for name in ("tc_longest_palindrome", "tc_longest_palindrome_dev"):
        assert longest(name, m=17) == TC_ERR_ARG
        assert longest(name, comp=_p(bad)) == TC_ERR_ARG
        assert longest(name, text=None) == TC_ERR_ARG
        assert longest(name, n=TC_MAX_N // 2 + 1) == TC_ERR_ARG
        for out in ((1, 2), (0, 2), (0, 1)):
            assert longest(name, out=out) == TC_ERR_ARG
        assert all(w.value == 0xDEADBEEF for w in words)
    assert longest("tc_longest_palindrome", text=None, n=0) == 0 and [w.value for w in words] == [0, 0, 0]
    assert call(m=16)[0] == 0
    rc, npal = call()
    assert rc == 0 and npal.value == len(_ref(tb.tobytes())[0]) and npal.value >= n
    with pytest.raises(Exception):
        ctx.palindromes(b"abcabc", max_mismatch=17)
    with pytest.raises(Exception):
        ctx.palindromes(b"abcabc", comp=bad)


def test_same_answer_twice_and_from_two_contexts(ctx):
    import textcomp
    rng = np.random.default_rng(0x9b50)
    t1, t2 = R.fibonacci(16) + b"q" + R.fibonacci(15), bytes(R.planted(rng, 2000, R.DNA))
    with textcomp.Context(0) as other:
        assert _dbg(other, "tc_dbg_fm_set_lcp_fanout", 4) == 0      # a setting of one context is not the other's
        a1 = ctx.palindromes(t1, None, 2)
        b2 = other.palindromes(t2, R.DNA, 1)
        b1 = other.palindromes(t1, None, 2)
        a2 = ctx.palindromes(t2, R.DNA, 1)
        again = ctx.palindromes(t1, None, 2)
        l1 = ctx.longest_palindrome(t1, None, 2)
        l2 = other.longest_palindrome(t1, None, 2)
    for got, what in ((a1, "ctx"), (again, "ctx again"), (b1, "other")):
        _same(got, _ref(t1, None, 2), what)
    for got, what in ((a2, "ctx"), (b2, "other")):
        _same(got, _ref(t2, R.DNA, 1), what)
    assert l1 == l2 == _longest_of(_ref(t1, None, 2))
