"""The directory of live parents of the aligned MSD level (csrc/tc_msd.hpp: msd_partition_dir_kernel, csrc/tc_msd_dir.hpp;
TC_MSD_DIR): level 3 with the joint table keeps its workgroup's live parents in LDS, its tile cursor reads LDS only, and
the next parent's digit rows wait in an LDS shadow.  Every case is encoded with TC_MSD_DIR=1 and with TC_MSD_DIR=0 in one
context and the two blocks must be equal byte for byte; up to 2^22 the block is also compared with the oracle;
tc_stats.msd_path and tc_dbg_msd_dir (include/textcomp_debug.h) say which way the case went.  The mechanics are those of
tests/test_gpu_msd_split.py.

The case with parents of several full tiles is sigma = 3 at 168 000 000 bytes, not sigma = 2 at 2^25, which does not take
the key-only way (see the test)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    c.lib.tc_dbg_msd_dir.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    c.lib.tc_dbg_msd_dir.restype = C.c_int
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _msd_for_small_records(monkeypatch):
    monkeypatch.setenv("TC_SA_MSD_MIN_LOG2", "10")


def _dir(ctx):
    """(used, fills) of the context's last suffix sort"""
    out = (C.c_uint32 * 2)(7, 7)
    assert ctx.lib.tc_dbg_msd_dir(ctx.handle, out) == 0
    assert out[0] in (0, 1)
    return int(out[0]), int(out[1])


def _workgroups():
    import torch
    return min(256, torch.cuda.get_device_properties(0).multi_processor_count)


def _oracle_block(t):
    L = O.bwt_encode_arr(t)
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return dict(primary=int(np.nonzero(L < 0)[0][0]), final_list=fl.tolist(), run_count=counts, run_value=vals)


def _assert_block(blk, want, what):
    assert blk["primary"] == want["primary"], what
    assert list(blk["final_list"]) == list(want["final_list"]), what
    assert np.array_equal(blk["run_count"], want["run_count"]) and np.array_equal(blk["run_value"], want["run_value"]), what


def _check(ctx, t, monkeypatch, used=1, keyonly=1, oracle=True):
    """both settings in one context; returns (stats, fills) of the TC_MSD_DIR=1 encode"""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    monkeypatch.setenv("TC_MSD_DIR", "1")
    blk = ctx.encode(t)
    st = ctx.stats()
    got = (st.msd_path, st.msd_keyonly) + _dir(ctx)
    monkeypatch.setenv("TC_MSD_DIR", "0")
    ref = ctx.encode(t)
    st0 = ctx.stats()
    got0 = (st0.msd_path, st0.msd_keyonly) + _dir(ctx)
    monkeypatch.delenv("TC_MSD_DIR")
    print("n=%d: TC_MSD_DIR=1 (msd_path, keyonly, dir, fills) = %s, TC_MSD_DIR=0 %s" % (len(t), got, got0))
    assert blk["primary"] == ref["primary"] and list(blk["final_list"]) == list(ref["final_list"])   # byte for byte
    assert blk["run_count"].tobytes() == ref["run_count"].tobytes() and blk["run_value"].tobytes() == ref["run_value"].tobytes()
    if oracle:
        want = _oracle_block(t)
        _assert_block(blk, want, "TC_MSD_DIR=1 against the oracle")
        _assert_block(ref, want, "TC_MSD_DIR=0 against the oracle")
        assert ctx.decode(blk) == t.tobytes()
    assert got[0] == 1 and got0[0] == 1 and got[1] == keyonly and got0[1] == keyonly, (got, got0)
    assert got[2] == used and got0[2:] == (0, 0), (got, got0)
    assert (got[3] >= 1) if used else (got[3] == 0), got
    return st, got[3]


@pytest.mark.parametrize("n", [1100, 8191, 8192, 100003, (1 << 22) + 5])
def test_dir_iid_acgtn_lengths(ctx, n, monkeypatch):
    """less than a tile (a key or two per parent: every workgroup still owns some); N = n + 1 on both sides of a tile; 100003: about 6 keys per parent,
    every tile is the last of its segment and the look-ahead crosses three parents each time; every workgroup with
    parents of several tiles"""
    _check(ctx, O.gen_acgtn(0xD1 + n, n), monkeypatch)


@pytest.mark.parametrize("sigma", [2, 3, 4])
def test_dir_small_alphabets_refill(ctx, sigma, monkeypatch):
    """the generator of tests/test_gpu_msd_split.py::test_split_other_small_alphabets: the live parents thin out and long
    stretches of slots are empty (sigma = 2: the first live parent is slot 31097), so some workgroup's first batch of
    slots finds nothing and it fills again: more fills than workgroups, which is at least the workgroups that own a parent"""
    rng = np.random.default_rng(sigma)
    alpha = rng.permutation(256)[:sigma]
    _, fills = _check(ctx, alpha[rng.integers(0, sigma, 100003)], monkeypatch)
    assert fills > _workgroups(), fills


def test_dir_parents_of_several_full_tiles(ctx, monkeypatch):
    """Parents of at least three full tiles, on / off only, and a round trip on the device.  The text: sigma = 3 iid at
    n = 168 000 000, made on the device -- 3^8 = 6561 level-3 parents of 25 606 +- 160 suffixes, three full tiles and a part.
    (Not sigma = 2 at 2^25: two symbols leave about N^2 / 2^35 suffixes tied on the whole key, and from 2^24 suffixes on
    that is more than the key-only levels are tried for -- csrc/tc_sa_plan.hpp: sa_round0_plan -- so its levels move suffix
    starts, measured: msd_keyonly = 0; below 2^24 its 1024 parents have two tiles.  Three symbols: about 1200 tied.)"""
    import torch
    from textcomp import Block
    n = 168_000_000
    g = torch.Generator(device="cuda")
    g.manual_seed(0xD2)
    alpha = torch.tensor([ord("c"), ord("a"), ord("t")], dtype=torch.uint8, device="cuda")
    d_text = alpha[torch.randint(0, 3, (n,), generator=g, device="cuda")]
    cap = n + 2

    def encode(v):
        monkeypatch.setenv("TC_MSD_DIR", v)
        cnt = torch.empty(cap, dtype=torch.int32, device="cuda")
        val = torch.empty(cap, dtype=torch.int16, device="cuda")
        b = Block()
        b.nruns, b.run_count, b.run_value = cap, cnt.data_ptr(), val.data_ptr()
        torch.cuda.synchronize()
        ctx._check(ctx.lib.tc_encode_dev(ctx.handle, C.c_void_p(d_text.data_ptr()), n, C.byref(b)))
        st = ctx.stats()
        return b, cnt, val, (st.msd_path, st.msd_keyonly) + _dir(ctx)

    b1, c1, v1, got = encode("1")
    b0, c0, v0, got0 = encode("0")
    monkeypatch.delenv("TC_MSD_DIR")
    print("sigma 3, n %d: TC_MSD_DIR=1 (msd_path, keyonly, dir, fills) = %s, TC_MSD_DIR=0 %s" % (n, got, got0))
    assert got[:3] == (1, 1, 1) and got[3] >= 1 and got0 == (1, 1, 0, 0), (got, got0)
    k = int(b1.nruns)
    assert (k, int(b1.primary), int(b1.sigma)) == (int(b0.nruns), int(b0.primary), int(b0.sigma))
    assert list(b1.final_list[:b1.sigma]) == list(b0.final_list[:b0.sigma])
    assert torch.equal(c1[:k], c0[:k]) and torch.equal(v1[:k], v0[:k])
    del c0, v0
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx._check(ctx.lib.tc_decode_dev(ctx.handle, C.byref(b1), C.c_void_p(back.data_ptr())))
    assert torch.equal(back, d_text)


def test_dir_end_marker_parents(ctx, monkeypatch):
    """a text that ends in a run of 30 symbols: the last suffixes' parents hold the end marker, one key each"""
    t = O.gen_acgtn(0xD3, 50000).copy()
    t[-30:] = ord("A")
    _check(ctx, t, monkeypatch)


def _sa_case(ctx, t, monkeypatch):
    want = O.suffix_array(t).astype(np.int64)
    for v in ("1", "0"):
        monkeypatch.setenv("TC_MSD_DIR", v)
        sa = ctx.suffix_array(t)
        st = ctx.stats()
        used, fills = _dir(ctx)
        print("suffix array n=%d TC_MSD_DIR=%s: msd_path %d keyonly %d dir %d fills %d" % (len(t), v, st.msd_path, st.msd_keyonly, used, fills))
        assert st.msd_path == 1 and st.msd_keyonly == 0
        assert (used, fills >= 1) == ((1, True) if v == "1" else (0, False))
        assert np.array_equal(sa.astype(np.int64), want), "TC_MSD_DIR=" + v
    monkeypatch.delenv("TC_MSD_DIR")


def test_dir_suffix_array_small_directory(ctx, monkeypatch):
    """tc_suffix_array moves suffix starts: the instance with values and its directory of 128 entries (50000 ACGTN
    suffixes: about 3 keys per parent, one tile each)"""
    _sa_case(ctx, O.gen_acgtn(0xD4, 50000), monkeypatch)


def test_dir_suffix_array_more_live_parents_than_entries(ctx, monkeypatch):
    """the same text on 16 workgroups (TC_MSD_GRID): each owns about 980 live parents and a batch of 1024 slots holds up to
    500, against 128 entries -- a round of a fill finds more than fits and the next fill starts at the first slot left out.
    (An alphabet with denser slots has no joint table, hence no aligned level: more than 128 digits of real symbols.)"""
    monkeypatch.setenv("TC_MSD_GRID", "16")
    _sa_case(ctx, O.gen_acgtn(0xD4, 50000), monkeypatch)


def test_dir_suffix_array_sigma2(ctx, monkeypatch):
    """... and on the sigma = 2 text at 2^22: parents of 4096 keys, long empty stretches of slots"""
    rng = np.random.default_rng(0xD5)
    alpha = rng.permutation(256)[:2].astype(np.uint8)
    _sa_case(ctx, alpha[rng.integers(0, 2, 1 << 22)], monkeypatch)


def test_dir_is_not_used_without_the_joint_table(ctx, monkeypatch):
    """TC_SA_MSD_JOINT=0: no aligned level, so no directory whatever TC_MSD_DIR says; the block is exact"""
    monkeypatch.setenv("TC_SA_MSD_JOINT", "0")
    _check(ctx, O.gen_acgtn(0xD6, 100003), monkeypatch, used=0)
