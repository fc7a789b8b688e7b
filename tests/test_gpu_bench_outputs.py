"""bench.py at N = 1: a plain run does the timed steps only and prints the headline fields; --dump-outputs writes what the
timed path (tc_encode_dev) returned in its last step -- equal to the CPU oracle's encode of the same record, and the same
from run to run; --full adds the extra legs after the headline."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xC3                  # the N = 1 record of bench.py
LEGS = ("container", "host_path", "fm_count", "classes", "cpu_baseline")


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(a) for a in args], env=env,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def _slice_sums(want):
    """bench.dump_outputs's slice sums of a whole array, restated in numpy"""
    B = -(-len(want) // 4096)
    pad = np.zeros(4096 * B, np.int64)
    pad[:len(want)] = want
    w = np.arange(4096 * B, dtype=np.int64) % 65521 + 1
    return np.stack([pad.reshape(4096, B).sum(1), (pad * w).reshape(4096, B).sum(1)], axis=1).astype(np.float64)


def _oracle(n):
    L = O.bwt_encode_arr(O.gen_acgtn(SEED, n))
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return int(np.nonzero(L < 0)[0][0]), fl, counts, vals


def test_plain_run_is_lean_and_dumps_the_whole_block(tmp_path):
    n = 1 << 16
    out = _bench("--steps", 3, "--warmup", 1, "--n", n, "--dump-outputs", tmp_path)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "MB/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert abs(out["value"] - n / (out["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * out["value"] + 0.2
    assert not [k for k in LEGS if k in out], "a plain run ran an extra leg"
    got = _load(tmp_path)
    assert all(v.dtype == np.float64 for v in got.values())
    primary, fl, counts, vals = _oracle(n)
    assert got["primary"].tolist() == [primary] and got["nruns"].tolist() == [len(counts)]
    assert got["sigma"].tolist() == [len(fl)] and got["final_list"].tolist() == fl.tolist()
    assert np.array_equal(got["run_count"], counts) and np.array_equal(got["run_value"], vals)


def test_dump_of_a_long_record_is_reproducible_and_exact(tmp_path):
    n = 1 << 22              # ~3.4 M runs: each run array as a seeded sample + slice sums
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _bench("--steps", 2, "--warmup", 1, "--n", n, "--dump-outputs", a)
    _bench("--steps", 1, "--warmup", 0, "--n", n, "--dump-outputs", b)
    da, db = _load(a), _load(b)
    assert sorted(da) == sorted(db) and all(np.array_equal(da[k], db[k]) for k in da)
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(a, "*.npy"))) <= 64 << 20
    primary, fl, counts, vals = _oracle(n)
    assert da["primary"].tolist() == [primary] and da["final_list"].tolist() == fl.tolist()
    assert da["nruns"].tolist() == [len(counts)]
    for name, want in (("run_count", counts), ("run_value", vals)):
        idx = da[name + "_index"].astype(np.int64)
        assert len(idx) > 200000 and np.array_equal(da[name + "_sample"], want[idx])
        assert np.array_equal(da[name + "_slice_sums"], _slice_sums(want))


def test_full_run_adds_the_legs():
    out = _bench("--steps", 2, "--warmup", 1, "--n", 1 << 24, "--cpu-sample", 1 << 20, "--full")
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    for k in ("container", "host_path", "cpu_baseline"):     # (fm_count and classes: at the 1 GiB record only)
        assert k in out and "error" not in out[k], (k, out.get(k))
    assert out["host_path"]["pageable"]["identical_to_device_path"]


def test_two_rank_rehearsal_dumps_the_gathered_containers(tmp_path):
    """N > 1 (two ranks on the one GPU, exchange over gloo): what rank 0 received in the last step, every rank's container,
    equal to the container this process encodes from that rank's record (seed 0xC500 + rank); a plain run does not decode
    them (containers_verified 0: that check is --full's)"""
    import ctypes as C
    import torch
    import textcomp
    n = 1 << 20
    env = dict(os.environ, TC_BENCH_REHEARSAL="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--n", str(n), "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert out["steps"] == 2 and out["gather"]["containers_verified"] == 0
    got = _load(tmp_path)
    assert got["container_bytes"].tolist() == out["gather"]["container_bytes"]
    assert len(out["gather"]["container_bytes"]) == 2
    ctx = textcomp.Context(0)
    try:
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        pcap = n + n // 4 + 4096
        buf = torch.empty(pcap, dtype=torch.uint8, device="cuda")
        for r, nb in enumerate(out["gather"]["container_bytes"]):
            assert ctx.lib.tc_generate_dev(ctx.handle, 0, 0xC500 + r, n, C.c_void_p(d_text.data_ptr())) == 0
            used = ctx.encode_container_dev(d_text.data_ptr(), n, buf.data_ptr(), pcap)
            assert used == nb
            want = buf[:used].cpu().numpy()
            idx = got["container_rank%d_index" % r].astype(np.int64)
            assert len(idx) > 100000 and np.array_equal(got["container_rank%d_sample" % r], want[idx])
            assert np.array_equal(got["container_rank%d_slice_sums" % r], _slice_sums(want))
    finally:
        ctx.close()
