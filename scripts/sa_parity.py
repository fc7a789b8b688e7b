#!/usr/bin/env python3
"""Parity listing of the suffix-sort driver (csrc/tc_sa_host.hpp): per case one line `label sha256 fingerprint` for
tc_suffix_array and one for tc_bwt_encode_dev (which passes no array, so the key-only MSD levels are eligible).  The hash
is over the return code and the raw output bytes (the suffix array; the last column and the primary); the fingerprint
is what tc_stats says about the path that call took: sigma, rounds, m / passes / h / key_bytes up to rounds,
keygen_fused, finish_pass, sample_dups, msd_path, msd_keyonly, seg_rounds, chain_rounds.  Two builds of the library took
the same path through the host logic and computed the same bytes exactly when their listings are equal:

  python scripts/sa_parity.py > new.txt
  python scripts/sa_parity.py --lib OLD.so > old.txt && diff old.txt new.txt

The cases are the smallest at which each branch of the driver is entered, and the script asserts the statistic that
shows it was.  The fingerprint is meant to change when a selector is tuned on purpose: then the listing under
profiles/ is made anew; it is no test golden."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "text-compression_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def with_copies(t, seed, count, lo, hi):
    """the copy loop of tests/test_gpu_msd.py: `count` stretches of lo .. hi - 1 symbols copied elsewhere"""
    rng = np.random.default_rng(seed)
    t = np.array(t, dtype=np.uint8)
    for _ in range(count):
        ln = int(rng.integers(lo, hi)) if hi > lo else lo
        a, b = int(rng.integers(0, len(t) - ln)), int(rng.integers(0, len(t) - ln))
        t[b:b + ln] = t[a:a + ln].copy()
    return t


def small_alphabet(sigma, n, seed):
    rng = np.random.default_rng(seed)
    alpha = np.sort(rng.permutation(256)[:sigma]).astype(np.uint8)
    return alpha[rng.integers(0, sigma, n)]


def poly_a_and_family():
    """tests/test_gpu_msd.py, test_msd_big_instance_keeps_long_buckets"""
    rng = np.random.default_rng(99)
    n = 600000
    acgt = np.frombuffer(b"ACGT", np.uint8)
    t = acgt[rng.integers(0, 4, n)].copy()
    t[1000:13000] = ord("A")
    fam = acgt[rng.integers(0, 4, 300)]
    for _ in range(80):
        a = int(rng.integers(30000, n - 400))
        c = fam.copy()
        mut = rng.random(300) < 0.1
        c[mut] = acgt[rng.integers(0, 4, int(mut.sum()))]
        t[a:a + 300] = c
    return t


def cases():
    """(label, text, environment, check(st_sa, st_bwt) or None)"""
    import oracle as O
    import classgen
    from test_gpu_encode import _genome_like
    MSD = {"TC_SA_MSD_MIN_LOG2": "10"}
    iid = O.gen_acgtn(0xC2 + 100003, 100003)
    iid1m = O.gen_acgtn(0xC2 + (1 << 20) - 1, (1 << 20) - 1)
    genome = np.frombuffer(_genome_like(1, 200000, 500, 40, 120), np.uint8)
    few_ties = with_copies(O.gen_acgtn(77, 100003), 5, 6, 22, 120)
    copies = with_copies(O.gen_acgtn(77, 400000), 5, 40, 22, 300)
    keyonly = with_copies(small_alphabet(5, 400000, 17), 18, 30, 22, 300)
    thousand = with_copies(O.gen_acgtn(5, 600000), 23, 20, 1000, 1000)
    poly20k = O.gen_acgtn(78, 300000).copy()
    poly20k[1000:21000] = ord("A")
    big = with_copies(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(300004).integers(0, 4, 300000)], 6, 20, 22, 200)
    zipf = classgen.zipf_words(1 << 20)
    periodic = np.resize(np.random.default_rng(7).integers(0, 4, 4096).astype(np.uint8) + 65, 30000)
    stretch = O.gen_acgtn(9, 100003).copy()      # a periodic stretch inside iid text: few enough ties for sparse ranks
    stretch[40000:46000] = np.resize(periodic[:700], 6000)
    ascii17 = small_alphabet(17, 100003, 3)
    both = lambda f: (lambda a, b: f(a) and f(b))
    return [
        ("empty", np.zeros(0, np.uint8), {}, None),
        ("one-byte", np.array([66], np.uint8), {}, None),
        ("unary", np.full(5000, 65, np.uint8), {}, both(lambda s: s.sigma == 2 and s.rounds == 0)),
        ("lsd-nothing-tied", iid, {}, both(lambda s: s.finish_pass == 1 and s.rounds == 1 and s.msd_path == 0)),
        ("lsd-tier2", genome, {}, both(lambda s: s.finish_pass == 1 and s.m[1] > 0)),
        ("lsd-tier2-off", genome, {"TC_SA_TIER2": "0"}, both(lambda s: s.finish_pass == 0)),
        ("tied-tiny", few_ties, {}, both(lambda s: s.finish_pass == 1 and 0 < s.m[1] <= 4096)),
        ("tied-tiny-off", few_ties, {"TC_SA_TINY": "0"}, both(lambda s: s.finish_pass == 1 and 0 < s.m[1] <= 4096)),
        ("msd-100003", iid, MSD, lambda a, b: a.msd_path == 1 and b.msd_path == 1 and a.msd_keyonly == 0 and b.msd_keyonly == 1),
        ("msd-2^20-1", iid1m, MSD, lambda a, b: a.msd_path == 1 and b.msd_path == 1 and a.msd_keyonly == 0 and b.msd_keyonly == 1),
        ("msd-sigma2", small_alphabet(2, 300000, 2), MSD, both(lambda s: s.msd_path == 1)),
        ("msd-sigma15", small_alphabet(15, 300000, 15), MSD, both(lambda s: s.msd_path == 1)),
        ("msd-keyonly-recovery", keyonly, MSD, lambda a, b: b.msd_path == 1 and b.msd_keyonly == 1 and b.rounds >= 2 and b.m[1] > 0),
        ("msd-rerun-with-starts", thousand, dict(MSD, TC_SA_MSD="2"), lambda a, b: b.msd_path == 1 and b.msd_keyonly == 0 and b.m[1] > (1 << 15)),
        ("msd-gives-way", poly20k, MSD, both(lambda s: s.msd_path == 0)),
        ("msd-big", big, dict(MSD, TC_SA_MSD_BIG="1"), both(lambda s: s.msd_path == 1 and s.rounds >= 2)),
        ("msd-big-keyround", poly_a_and_family(), dict(MSD, TC_SA_MSD_BIG="1", TC_SA_SEG_MIN="1"),
         both(lambda s: s.msd_path == 1 and s.rounds >= 3 and s.passes[1] == 1 and s.h[1] == 9 and s.seg_rounds >= 1)),
        ("full-forced", copies, {"TC_SA_FINISH": "0"}, both(lambda s: s.finish_pass == 0)),
        ("full-hopeless", zipf, {}, both(lambda s: s.sample_dups > 819 and s.finish_pass == 0)),
        ("full-hopeless-regions", zipf, {"TC_SA_BIN_MIN_LOG2": "0"}, both(lambda s: s.sample_dups > 819 and s.finish_pass == 0)),
        ("dense", copies, {"TC_SA_DENSE": "1"}, both(lambda s: s.finish_pass == 0 and s.rounds >= 2)),
        ("dense-regions", copies, {"TC_SA_DENSE": "1", "TC_SA_BIN_MIN_LOG2": "0"}, both(lambda s: s.finish_pass == 0 and s.rounds >= 2)),
        ("sparse-accel", genome, {"TC_SA_ACCEL_MIN": "1"}, both(lambda s: s.finish_pass == 1 and s.rounds >= 2)),
        ("sparse-accel-kdir-search", genome, {"TC_SA_ACCEL_MIN": "1", "TC_SA_KDIR_SEARCH": "1"}, both(lambda s: s.finish_pass == 1 and s.rounds >= 2)),
        ("sparse-accel-full", genome, {"TC_SA_ACCEL_MIN": "1", "TC_SA_FINISH": "0"}, both(lambda s: s.finish_pass == 0 and s.rounds >= 2)),
        ("rounds-segmented", genome, {"TC_SA_SEG_MIN": "1"}, both(lambda s: s.seg_rounds >= 1)),
        ("rounds-radix", genome, {"TC_SA_SEG": "0"}, both(lambda s: s.seg_rounds == 0 and s.rounds >= 2 and s.passes[1] > 1)),
        ("chain-dense", periodic, {"TC_SA_CHAIN": "2", "TC_SA_SEG_MIN": "1", "TC_SA_DENSE": "1"},
         both(lambda s: s.chain_rounds >= 1 and 2 in list(s.passes[1:s.rounds]))),
        ("chain-sparse", stretch, {"TC_SA_CHAIN": "2", "TC_SA_SEG_MIN": "1"},
         both(lambda s: s.chain_rounds >= 1 and s.finish_pass == 1 and 2 in list(s.passes[1:s.rounds]))),
        ("chain-periodic", periodic, {"TC_SA_CHAIN": "2", "TC_SA_SEG_MIN": "1"},
         both(lambda s: s.chain_rounds >= 1 and 2 in list(s.passes[1:s.rounds]))),
        ("keys-not-fused", iid, {"TC_KEYGEN_FUSED": "0"}, both(lambda s: s.keygen_fused == 0)),
        ("keys-no-onehist", iid, {"TC_KB_ONEHIST": "0"}, both(lambda s: s.keygen_fused == 0)),
        ("keys-17-symbols", ascii17, {}, both(lambda s: s.keygen_fused == 0 and s.sigma == 18)),
    ]


def fingerprint(st):
    r = int(st.rounds)
    arr = lambda a: ",".join(str(int(v)) for v in a[:r])
    return "sigma=%d rounds=%d m=[%s] passes=[%s] h=[%s] key_bytes=[%s] fused=%d finish=%d dups=%d msd=%d keyonly=%d seg=%d chain=%d" % (
        st.sigma, r, arr(st.m), arr(st.passes), arr(st.h), arr(st.key_bytes), st.keygen_fused, st.finish_pass, st.sample_dups,
        st.msd_path, st.msd_keyonly, st.seg_rounds, st.chain_rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build of libtextcomp.so")
    a = ap.parse_args()
    if a.lib:
        os.environ["TEXTCOMP_LIB"] = os.path.abspath(a.lib)
    import torch
    import textcomp

    def run(ctx, label, t):
        """both entry points on one text -> their statistics"""
        lib, n, out = ctx.lib, len(t), []
        sa = np.full(n + 1, 0x22222222, np.uint32)
        rc = lib.tc_suffix_array(ctx.handle, t.ctypes.data_as(C.c_void_p) if n else None, n, sa.ctypes.data_as(C.c_void_p))
        out.append(ctx.stats())
        print(label, "suffix_array", hashlib.sha256(b"rc=%d;" % rc + sa.tobytes()).hexdigest(), fingerprint(out[-1]), flush=True)
        d_text = torch.from_numpy(np.concatenate([t, np.zeros(16, np.uint8)])).cuda()
        d_L = torch.full((n + 1 + 16,), 0x22, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        prim = C.c_uint64(0x2222)
        rc = lib.tc_bwt_encode_dev(ctx.handle, C.c_void_p(d_text.data_ptr()), n, C.c_void_p(d_L.data_ptr()), C.byref(prim))
        out.append(ctx.stats())
        print(label, "bwt_encode_dev", hashlib.sha256(b"rc=%d;primary=%d;" % (rc, prim.value) + d_L[:n + 1].cpu().numpy().tobytes()).hexdigest(),
              fingerprint(out[-1]), flush=True)
        return out

    def with_env(env, fn):
        for k, v in env.items():
            os.environ[k] = v
        try:
            return fn()
        finally:
            for k in env:
                os.environ.pop(k, None)

    all_cases = cases()
    with textcomp.Context(0) as ctx:
        for label, t, env, check in all_cases:
            t = np.ascontiguousarray(t, dtype=np.uint8)
            sts = with_env(env, lambda: run(ctx, label, t))
            assert check is None or check(*sts), "%s: the branch was not entered" % label
    # the ticket trip: the first attempt of a fresh context's sort is abandoned, the retry gives the same outputs
    trip_text = np.ascontiguousarray(all_cases[3][1])
    with textcomp.Context(0) as ctx:
        sts = with_env({"TC_DBG_TICKET_TRIP": "1"}, lambda: run(ctx, "ticket-trip", trip_text))
        assert sts[0].ticket_fallbacks >= 1, "ticket-trip: no retry"


if __name__ == "__main__":
    main()
