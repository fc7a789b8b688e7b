"""The segmented sort of a doubling round (seg_sort_pairs: csrc/tc_sa_host.hpp, kernels in csrc/tc_seg.hpp) and
tied_small_kernel as the operations they are, through tc_dbg_seg_sort / tc_dbg_tied_small (include/textcomp_debug.h), on
the named inputs of tests/seg_ref.py.

Per case: every slot of the result is compared with seg_ref.seg_sort_ref (the keys exactly; the values as the same set
inside every stretch of equal keys), and the (long runs, tiles) the host read back before each partition level are those
of seg_ref.levels_ref -- a case built for the fourth level is seen to reach it on the device, a level too many or too
few fails even where the order comes out right.  What each case is for (its size classes, the window edge it sits on,
the network size, the depth) is asserted on the CPU from the same models (tests/test_seg_ref.py).  After the last case of
a family the same context encodes a short text exactly: its workspace is intact.

Not observable through the entry: which buffer held a slot before seg_small_kernel brought it home (only that the right
pair arrives), and whether a window's tiny runs went through the network or counted in LDS (both give the same order)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import seg_ref as S

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_INTERNAL = -1, -6
GOOD_TEXT = np.frombuffer(b"mississippi river banks " * 40, np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    with textcomp.Context(0) as c:
        c.lib.tc_dbg_seg_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        c.lib.tc_dbg_seg_sort.restype = C.c_int
        c.lib.tc_dbg_tied_small.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 3
        c.lib.tc_dbg_tied_small.restype = C.c_int
        yield c


@pytest.fixture(scope="module")
def good_block():
    L = O.bwt_encode_arr(GOOD_TEXT)
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return int(np.nonzero(L < 0)[0][0]), fl.tolist(), counts, vals


def _encode_intact(ctx, good_block):
    primary, fl, counts, vals = good_block
    blk = ctx.encode(GOOD_TEXT)
    assert blk["primary"] == primary and blk["final_list"].tolist() == fl
    assert np.array_equal(blk["run_count"], counts) and np.array_equal(blk["run_value"], vals)


def _seg_sort(ctx, keys, vals, rbits):
    k, v = keys.copy(), vals.copy()
    lev = np.full(16, 0xdeadbeef, np.uint32)
    rc = ctx.lib.tc_dbg_seg_sort(ctx.handle, k.ctypes.data, v.ctypes.data, len(k), rbits, lev.ctypes.data)
    return rc, k, v, lev.tolist()


def _where(keys, slot):
    """the run (of equal grp) and the window of a slot, for the failure message"""
    starts, sizes = S.runs_of(keys)
    r = int(np.searchsorted(starts, slot, "right")) - 1
    return "slot %d (run of %d members from slot %d, headed in window %d at its slot %d; the slot is slot %d of window %d)" % (
        slot, sizes[r], starts[r], starts[r] // S.SEG_SPAN, starts[r] % S.SEG_SPAN, slot % S.SEG_SPAN, slot // S.SEG_SPAN)


@pytest.mark.parametrize("name", list(S.CASES))
def test_seg_sort(ctx, good_block, name):
    c = S.CASES[name]
    rc, k, v, lev = _seg_sort(ctx, c.keys, c.vals, c.rbits)
    assert rc == 0, "%s: %s" % (name, ctx.lib.tc_last_error(ctx.handle))
    bad = S.seg_sort_mismatch(c.keys, c.vals, k, v)
    if bad is not None:
        rk, rv = S.seg_sort_ref(c.keys, c.vals)
        pytest.fail("%s (%s): first difference at %s: got key %#x value %d, expected key %#x (value %d in the reference's order)"
                    % (name, c.what, _where(c.keys, bad), int(k[bad]), int(v[bad]), int(rk[bad]), int(rv[bad])))
    want = S.levels_words(S.model(name)[0])
    assert lev == want, "%s (%s): (long runs, tiles) per level %s, the model says %s" % (name, c.what, lev, want)
    if name == S.FAMILY_LAST[c.family]:
        _encode_intact(ctx, good_block)


def _tied(ctx, c):
    m = len(c.idx)
    slot, idx, grp = c.slot.copy(), c.idx.copy(), c.grp.copy()
    t = [np.full(m, 0xdeadbeef, np.uint32) for _ in range(3)]
    rc = ctx.lib.tc_dbg_tied_small(ctx.handle, c.mode, slot.ctypes.data, idx.ctypes.data, grp.ctypes.data, m,
                                   *[(a.ctypes.data if c.mode == 1 else None) for a in t])
    return rc, (slot, idx, grp), t


@pytest.mark.parametrize("m", S.TIED_M)
def test_tied_small(ctx, good_block, m):
    for name, c in S.TIED_CASES.items():
        if len(c.idx) != m:
            continue
        rc, inout, t = _tied(ctx, c)
        assert rc == 0, "%s: %s" % (name, ctx.lib.tc_last_error(ctx.handle))
        if c.mode == 0:
            bad = S.tied_small_mismatch(0, c.slot, c.idx, c.grp, inout)
        else:
            bad = S.tied_small_mismatch(1, c.slot, c.idx, c.grp, t)
            for a, b in zip(inout, (c.slot, c.idx, c.grp)):
                assert np.array_equal(a, b), "%s: mode 1 changed its input" % name
        assert bad is None, "%s (%s): %s" % (name, c.what, bad)
    if m == S.TIED_M[-1]:
        _encode_intact(ctx, good_block)


def test_bad_arguments_are_refused_and_the_context_goes_on(ctx, good_block):
    c = S.CASES["total_m65_last16"]
    k, v = c.keys.copy(), c.vals.copy()
    lev = np.zeros(16, np.uint32)
    f = ctx.lib.tc_dbg_seg_sort
    K, V, LV = k.ctypes.data, v.ctypes.data, lev.ctypes.data
    assert f(ctx.handle, K, V, 0, 32, LV) == TC_ERR_ARG
    assert f(ctx.handle, K, V, (1 << 24) + 1, 32, LV) == TC_ERR_ARG
    assert f(ctx.handle, K, V, len(k), 0, LV) == TC_ERR_ARG
    assert f(ctx.handle, K, V, len(k), 33, LV) == TC_ERR_ARG
    assert f(ctx.handle, None, V, len(k), 32, LV) == TC_ERR_ARG
    assert f(ctx.handle, K, None, len(k), 32, LV) == TC_ERR_ARG
    assert f(ctx.handle, K, V, len(k), 32, None) == TC_ERR_ARG
    assert f(None, K, V, len(k), 32, LV) == TC_ERR_ARG
    assert f(ctx.handle, K, V, len(k), 8, LV) == TC_ERR_ARG            # ranks of 32 bits, 8 declared
    down = k[::-1].copy()
    assert f(ctx.handle, down.ctypes.data, V, len(k), 32, LV) == TC_ERR_ARG    # grp decreases
    assert np.array_equal(k, c.keys) and np.array_equal(v, c.vals)     # nothing ran
    t = S.TIED_CASES["tied1_m17"]
    g = ctx.lib.tc_dbg_tied_small
    a = [x.copy() for x in (t.slot, t.idx, t.grp)]
    o = [np.zeros(4097, np.uint32) for _ in range(3)]
    A, Z = [x.ctypes.data for x in a], [x.ctypes.data for x in o]
    assert g(ctx.handle, 2, A[0], A[1], A[2], 17, *Z) == TC_ERR_ARG
    assert g(ctx.handle, -1, A[0], A[1], A[2], 17, *Z) == TC_ERR_ARG
    assert g(ctx.handle, 0, A[0], A[1], A[2], 0, *Z) == TC_ERR_ARG
    big = [np.zeros(4097, np.uint32) for _ in range(3)]
    assert g(ctx.handle, 0, big[0].ctypes.data, big[1].ctypes.data, big[2].ctypes.data, 4097, *Z) == TC_ERR_ARG
    assert g(ctx.handle, 1, big[0].ctypes.data, big[1].ctypes.data, big[2].ctypes.data, 4097, *Z) == TC_ERR_ARG
    assert g(ctx.handle, 0, None, A[1], A[2], 17, *Z) == TC_ERR_ARG
    assert g(ctx.handle, 0, A[0], None, A[2], 17, *Z) == TC_ERR_ARG
    assert g(ctx.handle, 0, A[0], A[1], None, 17, *Z) == TC_ERR_ARG
    assert g(ctx.handle, 1, A[0], A[1], A[2], 17, None, Z[1], Z[2]) == TC_ERR_ARG
    assert g(ctx.handle, 1, A[0], A[1], A[2], 17, Z[0], Z[1], None) == TC_ERR_ARG
    assert g(None, 0, A[0], A[1], A[2], 17, *Z) == TC_ERR_ARG
    # the context is as usable as before: both entries, and an encode
    rc, k2, v2, lev2 = _seg_sort(ctx, c.keys, c.vals, c.rbits)
    assert rc == 0 and S.seg_sort_mismatch(c.keys, c.vals, k2, v2) is None and lev2 == [0] * 16
    rc, _, tt = _tied(ctx, t)
    assert rc == 0 and S.tied_small_mismatch(1, t.slot, t.idx, t.grp, tt) is None
    _encode_intact(ctx, good_block)
