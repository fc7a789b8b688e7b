"""The minimal absent words of a text (tc_absent_words, tc_absent_word_profile and their _dev forms) against the reference of
tests/maw_ref.py (the row rule by monotonic stacks and prefix counts; tests/test_maw_ref.py holds it to brute force over all
substrings).  Everything is compared exactly -- the three arrays in the documented row order, the count, the histogram and its
total -- through the host and the _dev entries, on the smallest shapes at which the kernels can go wrong: alphabets on both sides
of the switch between the one-word and the four-word set (64 / 65 distinct bytes), every byte once (256 children under the root,
the largest output of one lane), a unique first byte (a child that is the primary row alone), a text that ends in a repeat with
one right extension (the dropped first child), row counts on both sides of a group of the two trees at the default fan-out and
at fan-out 4 and of two tiles of the count and fill passes, and the window / capacity / sizes-only / error protocol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import maw_ref as M

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "text-compression_amd", "csrc", "tc_fm_ms.hpp")).read()
MAW_TILE = int(re.search(r"#define FM_MS_NT (\d+)\n#define FM_MS_KERNEL __global__", _SRC).group(1))   # rows per workgroup of maw_row_kernel
KMAX = 24


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(t):
    """(left, pos, len) of a text under the window (2, 0), computed once; a window is a filter of it that keeps the order"""
    t = bytes(t)
    if t not in _REF:
        _REF[t] = M.absent_words(t)
    return _REF[t]


def _window(want, min_len, max_len):
    keep = (want[2] >= min_len) & ((want[2] <= max_len) if max_len else True)
    return tuple(x[keep] for x in want)


def _text(seed, n, sigma):
    """n bytes over sigma byte values spread over 0 .. 255, every one of them present when n >= sigma"""
    rng = np.random.default_rng(seed)
    alpha = (np.arange(sigma) * 256 // sigma).astype(np.uint8)
    idx = rng.integers(0, sigma, n)
    idx[:min(n, sigma)] = rng.permutation(sigma)[:min(n, sigma)]
    return alpha[idx].tobytes()


def _dbg(ctx, name, value):
    fn = getattr(ctx.lib, name)                     # include/textcomp_debug.h
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int
    return fn(ctx.handle, value)


def _same(got, want, what):
    for name, g, w, dt in zip(("left", "pos", "len"), got, want, (np.uint8, np.uint32, np.uint32)):
        assert g.dtype == dt and len(g) == len(w), (what, name, len(g), len(w))
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s[%d] = %d, want %d" % (what, name, bad[0], g[bad[0]], w[bad[0]])


def _host_of(res):
    return (res[0].cpu().numpy(), res[1].cpu().numpy().astype(np.uint32), res[2].cpu().numpy().astype(np.uint32))


def _every_way(ctx, t, what="", min_len=2, max_len=0, profile=True):
    """the list through the host and the _dev entry, the sizes-only form, and the profile both ways"""
    import torch
    t = bytes(t)
    want = _window(_ref(t), min_len, max_len)
    tag = "%s n=%d window=(%d, %d)" % (what, len(t), min_len, max_len)
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    assert ctx.absent_word_count(t, min_len, max_len) == len(want[0]), tag
    _same(ctx.absent_words(t, min_len, max_len), want, tag + " host")
    _same(_host_of(ctx.absent_words_dev(d_text, min_len, max_len)), want, tag + " dev")
    if profile:
        full = _ref(t)[2]
        hist = np.bincount(full[full <= KMAX].astype(np.int64), minlength=KMAX + 1)
        h, total = ctx.absent_word_profile(t, KMAX)
        assert h.dtype == np.uint64 and h.astype(np.int64).tolist() == hist.tolist() and total == len(full), tag + " profile"
        dh, total = ctx.absent_word_profile_dev(d_text, KMAX)
        assert dh.cpu().numpy().tolist() == hist.tolist() and total == len(full), tag + " profile dev"


# ------------------------------------------------------------------------------------------------ texts
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"aa", b"ab", b"ba"):
        _every_way(ctx, t, repr(t))
    assert ctx.absent_word_count(b"") == 0
    left, pos, ln = ctx.absent_words(b"")
    assert len(left) == len(pos) == len(ln) == 0
    h, total = ctx.absent_word_profile(b"", 5)
    assert h.tolist() == [0] * 6 and total == 0


def test_worked_examples(ctx):
    import textcomp

    def words(t):
        _every_way(ctx, t, repr(t))
        return [w.decode() for w in textcomp.absent_word_bytes(t, *ctx.absent_words(t))]
    assert words(b"abaab") == ["aaa", "bab", "aaba", "bb"]
    left, pos, ln = ctx.absent_words(b"abaab")
    assert (bytes(left), pos.tolist(), ln.tolist()) == (b"abab", [2, 3, 0, 4], [3, 3, 4, 2])
    assert words(b"aaabaab") == ["aaaa", "baaa", "baaba", "bab", "bb"]
    left, pos, ln = ctx.absent_words(b"aaabaab")
    assert (bytes(left), pos.tolist(), ln.tolist()) == (b"abbbb", [0, 0, 1, 5, 6], [4, 4, 5, 3, 2])
    assert words(b"mississippi") == "ii mip pip pis missip sissis im mm pm sm mp sp ipi ppp ms ps isi sss".split()


@pytest.mark.parametrize("n", [3, 64, 257, 1000])
def test_unary_texts(ctx, n):
    """a^(n + 1) and nothing else: the one child that is the primary row alone, under the deepest node"""
    import textcomp
    t = b"a" * n
    _every_way(ctx, t, "unary")
    assert textcomp.absent_word_bytes(t, *ctx.absent_words(t)) == [b"a" * (n + 1)]
    _every_way(ctx, t, "unary", 2, n, profile=False)            # the window cuts it
    _every_way(ctx, t, "unary", n + 1, n + 1, profile=False)    # and keeps it


@pytest.mark.parametrize("sigma", [2, 5, 64, 65, 256])
def test_alphabets_on_both_sides_of_the_set_width(ctx, sigma):
    for n in (300, 1500):
        _every_way(ctx, _text(0x3a00 + sigma, n, sigma), "random over %d" % sigma)


def test_all_bytes_once(ctx):
    """65 281 words of length 2 from 256 lanes: every root child lacks 255 left bytes, but for the pairs that occur"""
    t = M.all_bytes()
    _every_way(ctx, t, "all bytes")
    left, pos, ln = ctx.absent_words(t)
    assert len(left) == 65281 and (ln == 2).all()
    assert ctx.absent_word_count(t, 3, 0) == 0
    _every_way(ctx, t + t, "all bytes twice")


def test_unique_first_byte_and_dropped_first_child(ctx):
    import textcomp
    t = b"Z" + M.random_text(0x3b01, 400, 3)            # the primary row is a child of the root on its own: Lc is empty
    _every_way(ctx, t, "unique first byte")
    w = textcomp.absent_word_bytes(t, *ctx.absent_words(t))
    assert b"ZZ" in w and all(x + b"Z" in w for x in (b"a", b"c", b"g") if x in t)
    for t in (b"abcXabcYabc", b"abXab", M.random_text(0x3b02, 300, 2) + b"gattaca" * 2):
        _every_way(ctx, t, "ends in a repeat")          # w = the repeated suffix: its first child is w at the text's end
    _every_way(ctx, M.fibonacci(1000), "fibonacci")
    for p in (2, 3, 7):
        _every_way(ctx, M.periodic(700, p) + b"z" + M.periodic(300, p), "period %d twice" % p)


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097, 2 * MAW_TILE - 2, 2 * MAW_TILE - 1, 2 * MAW_TILE, 2 * MAW_TILE + 1])
def test_rows_at_group_and_tile_boundaries(ctx, n):
    """n and N = n + 1 on both sides of a group of the default fan-out (64), of a second-level group (4096) and of two tiles
    of the count and fill passes"""
    for sigma in (3, 70):
        _every_way(ctx, _text(0x3c00 + 7 * n + sigma, n, sigma), "random over %d" % sigma, profile=n < 1000)


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025])
def test_fanout_4(ctx, n):
    """trees of 4 to 6 levels over both set widths, and the texts whose nearest smaller rows are far"""
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        _every_way(ctx, b"a" * n, "unary, fan-out 4", profile=False)
        _every_way(ctx, M.periodic(n, 3), "period 3, fan-out 4", profile=False)
        _every_way(ctx, M.fibonacci(n), "fibonacci, fan-out 4")
        for sigma in (2, 4, 65, 256):
            _every_way(ctx, _text(0x3d00 + n + sigma, n, sigma), "random over %d, fan-out 4" % sigma)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0


def test_windows_cut_none_some_and_all(ctx):
    t = M.random_text(0x3e01, 3000, 4)
    full = _ref(t)
    longest, shortest = int(full[2].max()), int(full[2].min())
    assert longest >= 10 and shortest <= 6
    for lo, hi in ((2, 0), (2, longest), (shortest + 1, 0), (2, longest - 1), (7, 9), (longest, longest), (longest + 1, 0),
                   (2, 2), (0xffffffff, 0), (5, 0xffffffff)):
        _every_way(ctx, t, "windows", lo, hi, profile=False)
    assert 0 < len(_window(full, 7, 9)[0]) < len(full[0]) and len(_window(full, longest + 1, 0)[0]) == 0


# ------------------------------------------------------------------------------------------------ errors and protocol
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _call(lib, h, name, text, n, min_len, max_len, left, pos, ln, nmaw):
    return getattr(lib, name)(h, text, n, min_len, max_len, left, pos, ln, C.byref(nmaw) if nmaw is not None else None)


def test_capacity_and_sizes_only_host(ctx):
    lib, h = ctx.lib, ctx.handle
    t = M.random_text(0x3f01, 400, 3)
    tb = np.frombuffer(t, np.uint8)
    want = _ref(t)
    z = len(want[0])
    assert z >= 2
    nmaw = C.c_uint64(0)                            # sizes only
    assert _call(lib, h, "tc_absent_words", _p(tb), len(tb), 2, 0, None, None, None, nmaw) == 0 and nmaw.value == z
    a, b, c = np.full(z, 0xEE, np.uint8), np.full(z, 0xDEADBEEF, np.uint32), np.full(z, 0xDEADBEEF, np.uint32)
    nmaw = C.c_uint64(z - 1)                        # one too small: the count, nothing written
    assert _call(lib, h, "tc_absent_words", _p(tb), len(tb), 2, 0, _p(a), _p(b), _p(c), nmaw) == TC_ERR_CAPACITY and nmaw.value == z
    assert (a == 0xEE).all() and (b == 0xDEADBEEF).all() and (c == 0xDEADBEEF).all()
    nmaw = C.c_uint64(z)                            # exact
    assert _call(lib, h, "tc_absent_words", _p(tb), len(tb), 2, 0, _p(a), _p(b), _p(c), nmaw) == 0 and nmaw.value == z
    _same((a, b, c), want, "exact capacity")
    a2, b2, c2 = np.full(z + 5, 0xEE, np.uint8), np.full(z + 5, 0xDEADBEEF, np.uint32), np.full(z + 5, 0xDEADBEEF, np.uint32)
    nmaw = C.c_uint64(z + 5)                        # more: nothing behind the count is written
    assert _call(lib, h, "tc_absent_words", _p(tb), len(tb), 2, 0, _p(a2), _p(b2), _p(c2), nmaw) == 0 and nmaw.value == z
    _same((a2[:z], b2[:z], c2[:z]), want, "spare capacity")
    assert (a2[z:] == 0xEE).all() and (b2[z:] == 0xDEADBEEF).all() and (c2[z:] == 0xDEADBEEF).all()


def test_capacity_and_sizes_only_dev(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = M.random_text(0x3f02, 400, 3)
    want = _ref(t)
    z = len(want[0])
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    a = torch.full((z,), 0xEE, dtype=torch.uint8, device="cuda")
    b, c = (torch.full((z,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    pt, pa, pb, pc = (C.c_void_p(x.data_ptr()) for x in (d_text, a, b, c))
    nmaw = C.c_uint64(0)
    assert _call(lib, h, "tc_absent_words_dev", pt, len(t), 2, 0, None, None, None, nmaw) == 0 and nmaw.value == z
    nmaw = C.c_uint64(z - 1)
    assert _call(lib, h, "tc_absent_words_dev", pt, len(t), 2, 0, pa, pb, pc, nmaw) == TC_ERR_CAPACITY and nmaw.value == z
    assert bool((a == 0xEE).all()) and bool((b == -1).all()) and bool((c == -1).all())
    nmaw = C.c_uint64(z)
    assert _call(lib, h, "tc_absent_words_dev", pt, len(t), 2, 0, pa, pb, pc, nmaw) == 0 and nmaw.value == z
    _same(_host_of((a, b, c)), want, "exact capacity, dev")
    _same(_host_of(ctx.absent_words_dev(d_text, cap=1)), want, "the retry loop")    # a first capacity that is too small


def test_bad_arguments_and_edges(ctx):
    lib, h = ctx.lib, ctx.handle
    tb = np.frombuffer(b"abracadabra", np.uint8)
    n = len(tb)
    z = len(_ref(tb.tobytes())[0])
    a, b, c = np.full(z, 0xEE, np.uint8), np.full(z, 0xDEADBEEF, np.uint32), np.full(z, 0xDEADBEEF, np.uint32)

    def call(text=_p(tb), n=n, min_len=2, max_len=0, left=_p(a), pos=_p(b), ln=_p(c), cap=z, name="tc_absent_words"):
        nmaw = C.c_uint64(cap) if cap is not None else None
        return _call(lib, h, name, text, n, min_len, max_len, left, pos, ln, nmaw), nmaw

    for name in ("tc_absent_words", "tc_absent_words_dev"):     # (argument errors come before any buffer is touched)
        assert call(min_len=1, name=name)[0] == TC_ERR_ARG and call(min_len=0, name=name)[0] == TC_ERR_ARG
        assert call(min_len=5, max_len=4, name=name)[0] == TC_ERR_ARG and call(min_len=3, max_len=2, name=name)[0] == TC_ERR_ARG
        assert call(text=None, name=name)[0] == TC_ERR_ARG
        assert call(n=TC_MAX_N + 1, name=name)[0] == TC_ERR_ARG
        assert call(cap=None, name=name)[0] == TC_ERR_ARG
        assert call(left=None, name=name)[0] == TC_ERR_ARG and call(pos=None, name=name)[0] == TC_ERR_ARG
        assert call(ln=None, name=name)[0] == TC_ERR_ARG
        assert call(left=None, pos=None, ln=None, name=name)[0] == TC_ERR_ARG           # a capacity without buffers
        assert call(min_len=1, left=None, pos=None, ln=None, cap=0, name=name)[0] == TC_ERR_ARG     # in the sizes-only form too
        rc, nmaw = call(text=None, n=0, name=name)              # n = 0: nothing read, no words
        assert rc == 0 and nmaw.value == 0
    assert (a == 0xEE).all() and (b == 0xDEADBEEF).all() and (c == 0xDEADBEEF).all()
    rc, nmaw = call(min_len=4, max_len=4)
    assert rc == 0 and nmaw.value == int((_ref(tb.tobytes())[2] == 4).sum())
    with pytest.raises(Exception):
        ctx.absent_words(b"abc", min_len=1)
    with pytest.raises(Exception):
        ctx.absent_words(b"abc", min_len=4, max_len=3)
    hist = np.zeros(8, np.uint64)
    prof = lib.tc_absent_word_profile
    for kmax in (0, 1, 4097):
        assert prof(h, _p(tb), n, kmax, _p(hist), None) == TC_ERR_ARG
    assert prof(h, _p(tb), n, 5, None, None) == TC_ERR_ARG and prof(h, None, n, 5, _p(hist), None) == TC_ERR_ARG
    assert prof(h, _p(tb), n, 7, _p(hist), None) == 0            # total may be null
    assert hist.tolist() == M.profile(tb.tobytes(), 7)[0].tolist()
    h4096, total = ctx.absent_word_profile(tb.tobytes(), 4096)
    assert int(h4096.sum()) == total == z


def test_two_contexts_interleaved(ctx):
    import textcomp
    t1, t2 = M.random_text(0x3f11, 500, 2), _text(0x3f12, 600, 80)
    with textcomp.Context(0) as other:
        assert _dbg(other, "tc_dbg_fm_set_lcp_fanout", 4) == 0      # a setting of one context is not the other's
        a1 = ctx.absent_words(t1)
        b2 = other.absent_words(t2)
        p1 = ctx.absent_word_profile(t1, KMAX)
        a2 = other.absent_words(t2, 3, 5)
        c1 = ctx.absent_word_count(t1, 3, 0)
        p2 = other.absent_word_profile(t2, KMAX)
    _same(a1, _ref(t1), "ctx")
    _same(b2, _ref(t2), "other")
    _same(a2, _window(_ref(t2), 3, 5), "other, window")
    assert c1 == len(_window(_ref(t1), 3, 0)[0])
    for (hh, total), t in ((p1, t1), (p2, t2)):
        want, wt = M.profile(t, KMAX)
        assert hh.tolist() == want.tolist() and total == wt


def test_repeats_before_and_after_on_the_shared_workspace(ctx):
    """the calls share the context's workspace with tc_repeats: neither leaves anything the other trips over"""
    import rep_ref as R
    t = M.random_text(0x3f21, 2000, 4)
    want = R.repeats(t, R.MAXIMAL)
    before = ctx.repeats(t, with_sa=True)
    _every_way(ctx, t, "between two repeats calls")
    _every_way(ctx, _text(0x3f22, 5000, 100), "a larger text, wide sets", profile=False)
    after = ctx.repeats(t, with_sa=True)
    for g1, g2, w in zip(before, after, want):
        assert np.array_equal(g1, w) and np.array_equal(g2, w)
