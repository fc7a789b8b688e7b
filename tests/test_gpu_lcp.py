"""Suffix array and LCP array on the device (tc_lcp_array, tc_suffix_array_dev + tc_lcp_array_dev, tc_lcp_summary_dev)
against tests/lcp_ref.py, exactly.  Every text goes through both entry paths: the host form, and the two `_dev` calls
on tensors.  The shapes are the smallest at which each kernel can go wrong: the wide-load tails at the end of the text,
positions without a byte in front, values one below / on / above the short cap, a long item, a scan over several tiles
with an odd remainder, many workgroups.  The long-compare kernel's turn geometry, the short cap moved, and malformed
suffix arrays through the library are test_gpu_lcp_long.py (host/check/lcp_kernels.cpp walks the same malformed arrays
under a host sanitizer first)."""
import ctypes as C

import numpy as np
import pytest

import lcp_ref

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    with textcomp.Context(0) as c:
        yield c


def _dev_forms(ctx, text, offset=0):
    """suffix_array_dev + lcp_array_dev on a tensor view that starts `offset` bytes into its allocation"""
    import torch
    t = np.frombuffer(bytes(text), np.uint8)
    buf = torch.zeros(len(t) + offset, dtype=torch.uint8, device="cuda")
    d_text = buf[offset:]
    d_text.copy_(torch.from_numpy(t.copy()))
    assert offset == 0 or d_text.data_ptr() % 16 != 0
    d_sa = ctx.suffix_array_dev(d_text)
    d_lcp = ctx.lcp_array_dev(d_text, d_sa)
    return d_sa.cpu().numpy().view(np.uint32), d_lcp.cpu().numpy().view(np.uint32), d_lcp


def _check_both(ctx, text, sa_ref, lcp_ref_, offset=0):
    sa, lcp = ctx.lcp_array(text)
    assert np.array_equal(sa, sa_ref), "host form: suffix array"
    assert np.array_equal(lcp, lcp_ref_), "host form: LCP array, first difference at row %d" % int(np.flatnonzero(lcp != lcp_ref_)[:1].sum())
    sa_d, lcp_d, d_lcp = _dev_forms(ctx, text, offset)
    assert np.array_equal(sa_d, sa_ref), "_dev forms: suffix array"
    assert np.array_equal(lcp_d, lcp_ref_), "_dev forms: LCP array, first difference at row %d" % int(np.flatnonzero(lcp_d != lcp_ref_)[:1].sum())
    return d_lcp


def _random_text(rng, n, sigma):
    if sigma == 256:
        t = rng.integers(0, 256, n, dtype=np.uint8)
        if n >= 2:
            t[rng.integers(0, n)] = 0
            t[rng.integers(0, n)] = 255
        return t.tobytes()
    return np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, sigma, n)].tobytes()


@pytest.mark.parametrize("sigma", [2, 4, 5, 256])
def test_length_edges(ctx, sigma):
    rng = np.random.default_rng(0x1C90 + sigma)
    for n in EDGE_LENGTHS:
        text = _random_text(rng, n, sigma)
        sa_ref, l_ref = lcp_ref.esa_direct(text)
        assert l_ref[0] == 0 and (n == 0 or l_ref[1] == 0)
        _check_both(ctx, text, sa_ref, l_ref)


@pytest.mark.parametrize("offset", [1, 3, 5])
def test_misaligned_text(ctx, offset):
    rng = np.random.default_rng(0x1C91 + offset)
    for n in (17, 64, 257, 1000):
        text = _random_text(rng, n, 2)        # two letters: comparisons run over several 16-byte loads
        sa_ref, l_ref = lcp_ref.esa_direct(text)
        _check_both(ctx, text, sa_ref, l_ref, offset)


def test_values_around_the_short_cap(ctx):
    """two copies of a random block of c - 1, c, c + 1 and 4 c + 3 bytes with one distinct byte between them: the
    irreducible value of the second copy's start lands one below the cap, on it, and above it"""
    from textcomp import _lib
    c = _lib.TC_LCP_SHORT_CAP
    rng = np.random.default_rng(0x1C92)
    for m in (c - 1, c, c + 1, 4 * c + 3):
        block = _random_text(rng, m, 4)
        text = block + b"#" + block
        sa_ref, l_ref = lcp_ref.esa_direct(text)
        assert int(l_ref.max()) == m
        d_lcp = _check_both(ctx, text, sa_ref, l_ref)
        mx, row, tot = ctx.lcp_summary_dev(d_lcp)
        assert (mx, row, tot) == (m, int(np.argmax(l_ref)), int(l_ref.astype(np.uint64).sum()))


def test_unary_text_one_long_item_and_the_scan_over_many_tiles(ctx):
    n = 200_000
    text = b"A" * n
    sa_ref, l_ref = lcp_ref.unary_lcp(n)
    d_lcp = _check_both(ctx, text, sa_ref, l_ref)
    assert ctx.lcp_summary_dev(d_lcp) == (n - 1, n, (n - 1) * n // 2)


def _large_case(ctx, text):
    """larger texts: Kasai over the library's own suffix array (which the existing suite pins)"""
    sa_ref = ctx.suffix_array(text)
    l_ref = lcp_ref.kasai(text, sa_ref)
    return sa_ref, l_ref, _check_both(ctx, text, sa_ref, l_ref)


@pytest.mark.parametrize("period", [5, 4096])
def test_periodic_text(ctx, period):
    n = 3 * (1 << 16) + 1
    rng = np.random.default_rng(0x1C93 + period)
    block = b"ACGTN" if period == 5 else rng.integers(0, 4, period, dtype=np.uint8).tobytes()
    text = (block * (n // period + 1))[:n]
    sa_ref, l_ref, _ = _large_case(ctx, text)
    mask, val = lcp_ref.periodic_lcp_of_rows(sa_ref, n, period)      # the closed form, a second opinion
    assert mask.sum() >= n - 3 * period and np.array_equal(l_ref[mask], val[mask])


def test_fibonacci_word(ctx):
    a, b = b"a", b"ab"
    while len(b) < (1 << 17):
        a, b = b, b + a
    _large_case(ctx, b[:(1 << 17) + 1])


@pytest.mark.parametrize("kind,n", [(4, (1 << 17) + 3), (2, 1 << 18)])
def test_generated_classes(ctx, kind, n):
    """tc_generate_dev kind 4 (runs) and kind 2 (genome-like: its 300-bp repeats straddle the short cap)"""
    import torch
    d = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.lib.tc_generate_dev(ctx.handle, kind, 0x1C94 + kind, n, C.c_void_p(d.data_ptr())) == 0
    torch.cuda.synchronize()
    _large_case(ctx, d.cpu().numpy().tobytes())


def test_many_workgroups_and_the_summary(ctx):
    n = (1 << 20) + 1
    text = _random_text(np.random.default_rng(0x1C95), n, 4)
    _, l_ref, d_lcp = _large_case(ctx, text)
    mx, row, tot = ctx.lcp_summary_dev(d_lcp)
    assert mx == int(l_ref.max()) and row == int(np.argmax(l_ref)) and tot == int(l_ref.astype(np.uint64).sum())


def test_summary_ties_longest_repeat_and_distinct_substrings(ctx):
    import torch
    # a tie in the maximum: the smallest row; the sum exact
    for text in (b"abcabcxbcaybca", b"zz#zz#zz", b"ACGT", b"a", b"banana"):
        _, l_ref = lcp_ref.esa_direct(text)
        d_lcp = torch.from_numpy(l_ref.view(np.int32).copy()).cuda()
        assert ctx.lcp_summary_dev(d_lcp) == (int(l_ref.max()), int(np.argmax(l_ref)), int(l_ref.sum()))
    d = torch.tensor([0, 3, 1, 3, 3, 0], dtype=torch.int32, device="cuda")
    assert ctx.lcp_summary_dev(d) == (3, 1, 10)
    rng = np.random.default_rng(0x1C96)
    for n, sigma in ((1, 2), (2, 2), (57, 2), (130, 4), (200, 5), (200, 256)):
        text = _random_text(rng, n, sigma)
        a, b, length = ctx.longest_repeat(text)
        _, l_ref = lcp_ref.esa_direct(text)
        assert length == int(l_ref.max())
        if length:
            assert a != b and text[a:a + length] == text[b:b + length]
            assert a + length == n or b + length == n or text[a + length] != text[b + length]     # and no further
        assert ctx.distinct_substrings(text) == len({text[i:j] for i in range(n) for j in range(i + 1, n + 1)})


def test_argument_errors_answer_before_any_launch(ctx):
    import torch
    from textcomp import _lib
    lib, h = ctx.lib, ctx.handle
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = C.c_void_p(d.data_ptr())
    host = np.zeros(16, np.uint32)
    hp = host.ctypes.data_as(C.c_void_p)
    mx, row, tot = C.c_uint32(), C.c_uint64(), C.c_uint64()
    big = _lib.TC_MAX_N + 1
    assert lib.tc_suffix_array_dev(h, p, 4, None) == _lib.TC_ERR_ARG
    assert lib.tc_suffix_array_dev(h, None, 4, p) == _lib.TC_ERR_ARG
    assert lib.tc_suffix_array_dev(h, p, big, p) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array_dev(h, None, 4, p, p) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array_dev(h, p, 4, None, p) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array_dev(h, p, 4, p, None) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array_dev(h, p, big, p, p) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array(h, None, 4, hp, hp) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array(h, hp, 4, hp, None) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array(h, hp, big, hp, hp) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_summary_dev(h, None, 4, C.byref(mx), C.byref(row), C.byref(tot)) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_summary_dev(h, p, 0, C.byref(mx), C.byref(row), C.byref(tot)) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_summary_dev(h, p, 4, None, C.byref(row), C.byref(tot)) == _lib.TC_ERR_ARG
    assert lib.tc_lcp_array(None, hp, 4, hp, hp) == _lib.TC_ERR_ARG
    # the host form without a suffix array: the LCP array alone
    text = b"mississippi"
    lcp = np.empty(len(text) + 1, np.uint32)
    t = np.frombuffer(text, np.uint8)
    assert lib.tc_lcp_array(h, t.ctypes.data_as(C.c_void_p), len(t), None, lcp.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(lcp, lcp_ref.esa_direct(text)[1])
