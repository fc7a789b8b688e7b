"""The split key layout of the MSD round 0 (csrc/tc_msd.hpp, TC_MSD_SPLIT): when the levels move keys only and level 2's
joint count is on, level 1 stores every key as two 32-bit halves in two arrays, the joint count reads the high halves
alone (msd_count_hi_kernel) and level 2 reads both halves (msd_partition_split_kernel).  Every case encodes with the
split on and checks (a) the block against the oracle, the way tests/test_gpu_msd.py::_check checks an encode (the
suffix-array half of that check never takes key-only levels; test_suffix_array_keeps_the_old_layout covers it),
(b) that it is the block TC_MSD_SPLIT=0 gives for the same text in the same context, and (c) which way it went:
tc_stats.msd_path / msd_keyonly and tc_dbg_msd_split_used (include/textcomp_debug.h).


The shortest lengths are less than one 8192-key tile: the MSD way takes texts from 1024 suffixes on (msd_wanted,
csrc/tc_sa_host.hpp), one tile loaded pair by pair."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    c.lib.tc_dbg_msd_split_used.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    c.lib.tc_dbg_msd_split_used.restype = C.c_int
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _msd_for_small_records(monkeypatch):
    monkeypatch.setenv("TC_SA_MSD_MIN_LOG2", "10")


def _split_used(ctx):
    u = C.c_uint32(7)
    assert ctx.lib.tc_dbg_msd_split_used(ctx.handle, C.byref(u)) == 0
    assert u.value in (0, 1)
    return u.value


def _oracle_block(t):
    L = O.bwt_encode_arr(t)
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return dict(primary=int(np.nonzero(L < 0)[0][0]), final_list=fl.tolist(), run_count=counts, run_value=vals)


def _assert_block(blk, want, what):
    assert blk["primary"] == want["primary"], what
    assert list(blk["final_list"]) == list(want["final_list"]), what
    assert np.array_equal(blk["run_count"], want["run_count"]) and np.array_equal(blk["run_value"], want["run_value"]), what


def _check(ctx, t, monkeypatch, msd_path=1, keyonly=1, split=1, encode=None):
    """(a), (b), (c) of the module docstring; msd_path, keyonly, split: what is expected with TC_MSD_SPLIT=1"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    encode = encode or (lambda: ctx.encode(t))
    want = _oracle_block(t)
    monkeypatch.setenv("TC_MSD_SPLIT", "1")
    blk = encode()
    st = ctx.stats()
    got = (st.msd_path, st.msd_keyonly, _split_used(ctx))
    _assert_block(blk, want, "TC_MSD_SPLIT=1 against the oracle")                      # (a)
    if "n" in blk:
        assert ctx.decode(blk) == t.tobytes()
    monkeypatch.setenv("TC_MSD_SPLIT", "0")
    ref = encode()
    st0 = ctx.stats()
    got0 = (st0.msd_path, st0.msd_keyonly, _split_used(ctx))
    monkeypatch.delenv("TC_MSD_SPLIT")
    _assert_block(ref, want, "TC_MSD_SPLIT=0 against the oracle")
    assert blk["primary"] == ref["primary"] and list(blk["final_list"]) == list(ref["final_list"])   # (b): byte for byte
    assert blk["run_count"].tobytes() == ref["run_count"].tobytes() and blk["run_value"].tobytes() == ref["run_value"].tobytes()
    assert (got[0], got[2]) == (msd_path, split) and (got0[0], got0[2]) == (msd_path, 0), (got, got0)   # (c)
    if msd_path:
        assert got[1] == keyonly and got0[1] == keyonly, (got, got0)
    return st


@pytest.mark.parametrize("n", [1100, 8191, 8192, 32769, 32770, 32769 + 14, 32769 + 15, (1 << 22) + 5])
def test_split_iid_acgtn_lengths(ctx, n, monkeypatch):
    """far less than a tile; N = n + 1 on both sides of a tile boundary; N mod 16 around the 16-key store group and the
    rounding of a half to a 128-byte line; every workgroup with tiles and many segments that cross parents"""
    _check(ctx, O.gen_acgtn(0x5A + n, n), monkeypatch)


def test_split_text_pointer_off_by_one(ctx, monkeypatch):
    """the text one byte behind an aligned address on the device: level 1 takes its edge path (byte-wise loads) for
    every tile, together with the split stores"""
    import torch
    from textcomp import Block
    n = 100003
    t = O.gen_acgtn(0x5B, n)
    d = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d[1:n + 1] = torch.from_numpy(t).cuda()
    assert d.data_ptr() % 16 == 0
    cnt = torch.empty(n + 2, dtype=torch.int32, device="cuda")
    val = torch.empty(n + 2, dtype=torch.int16, device="cuda")

    def encode():
        b = Block()
        b.nruns, b.run_count, b.run_value = n + 2, cnt.data_ptr(), val.data_ptr()
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_encode_dev(ctx.handle, C.c_void_p(d.data_ptr() + 1), n, C.byref(b)))
        k = int(b.nruns)
        return dict(primary=int(b.primary), final_list=np.array(b.final_list[:b.sigma], dtype=np.int16),
                    run_count=cnt[:k].cpu().numpy().astype(np.uint32), run_value=val[:k].cpu().numpy().astype(np.uint16))
    _check(ctx, t, monkeypatch, encode=encode)


@pytest.mark.parametrize("sigma", [2, 3, 4, 5])
def test_split_other_small_alphabets(ctx, sigma, monkeypatch):
    """5 / 4 / 3 / 3 symbols per field in base sigma + 1: other field values, other rows of the joint table (32, 81, 64
    and 125 digits made of real symbols only); the generator of tests/test_gpu_msd.py::test_msd_other_small_alphabets"""
    rng = np.random.default_rng(sigma)
    alpha = rng.permutation(256)[:sigma]
    _check(ctx, alpha[rng.integers(0, sigma, 100003)], monkeypatch)


def test_split_end_marker_digits(ctx, monkeypatch):
    """a text that ends in a run of one symbol: the last suffixes' digits hold the end marker and are counted in the
    global joint table directly, not through the LDS rows"""
    t = O.gen_acgtn(0x5C, 50000).copy()
    t[-30:] = ord("A")
    _check(ctx, t, monkeypatch)


def test_split_gives_way_when_too_many_suffixes_are_tied(ctx, monkeypatch):
    """tests/test_gpu_msd.py::test_msd_keyonly_gives_way_when_too_many_suffixes_are_tied with the split on: the first
    attempt runs in the split layout, the levels then run again with suffix starts -- in the old layout -- and the block
    is exact"""
    monkeypatch.setenv("TC_SA_MSD", "2")
    rng = np.random.default_rng(23)
    n = 600000
    t = O.gen_acgtn(5, n).copy()
    for _ in range(20):
        ln = 1000
        a, b = int(rng.integers(0, n - ln)), int(rng.integers(0, n - ln))
        t[b:b + ln] = t[a:a + ln].copy()
    st = _check(ctx, t, monkeypatch, msd_path=1, keyonly=0, split=0)
    assert (1 << 15) < st.m[1] < 75000


def test_split_finish_with_a_digit_above_half_the_text(ctx, monkeypatch):
    """tests/test_gpu_msd.py::test_msd_keyonly_finish_with_a_digit_above_half_the_text with the split on: one digit pair
    holds most of the text, so one cell of the joint table counts more than 2^16 keys (32-bit cells: no overflow); the
    attempt ends with the LSD way as before, and the block is exact"""
    monkeypatch.setenv("TC_SA_MSD", "2")
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binary_long_run_128k.npz"))["text"]
    _check(ctx, t, monkeypatch, msd_path=0, split=0)


def test_split_is_not_used_without_the_joint_table(ctx, monkeypatch):
    monkeypatch.setenv("TC_SA_MSD_JOINT", "0")
    _check(ctx, O.gen_acgtn(0x5D, 100003), monkeypatch, split=0)


def test_suffix_array_keeps_the_old_layout(ctx, monkeypatch):
    """levels that move suffix starts (tc_suffix_array) never use the split layout"""
    monkeypatch.setenv("TC_MSD_SPLIT", "1")
    t = O.gen_acgtn(0x5E, 50000)
    sa = ctx.suffix_array(t)
    assert ctx.stats().msd_path == 1 and _split_used(ctx) == 0
    assert np.array_equal(sa.astype(np.int64), O.suffix_array(t).astype(np.int64))
