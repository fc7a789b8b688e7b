#!/usr/bin/env python3
"""The k-mers of a text from an enhanced suffix array that already lies in HBM: tc_kmers_esa_dev, tc_kmer_spectrum_esa_dev and
tc_kmer_profile_esa_dev, per input class and size, beside two yardsticks measured in the same run.

  python scripts/kmer_bench.py                         # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes
  python scripts/kmer_bench.py --kinds 0 --log2 26 --k 21

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/rep_bench.py); its suffix
array and LCP array are built once per class and size (tc_suffix_array_dev, tc_lcp_array_dev) and every k-mer call reads
them.  Times are HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has
drained: `--warmup` calls, then the median of `--steps` timed ones.  Every class and size runs in a child process of its own
under a time limit (`--limit` seconds); the parent never opens the device, and stops at the first child that fails.
  floor    tc_lcp_summary_dev over the same d_lcp: one 4-byte-per-row read, the floor of any pass            (yardstick a)
  rep+     tc_repeats_dev (maximal, min_len 1, min_occ 2, exact capacity) - sort - lcp: what the repeats add   (yardstick b)
One line per call: ms, ms / floor, the bytes the call has to move (lcp passes x 4 N + 4 per group head for sa + 12 per k-mer
written; the group count is taken from the (1, 0) list), those bytes per second beside the floor's, and the count."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))

NAMES = {0: "iid ACGTN", 1: "ascii96", 2: "genome-like", 3: "zipf words", 4: "runs", 5: "period 4096", 6: "assembly gaps"}
HEADER = "# class | log2 n | call | ms | x floor | MB moved | GB/s | count"


def child(a, kind, log2):
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib, h = ctx.lib, ctx.handle
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(h))

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    n = 1 << log2
    N = n + 1
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_sa = torch.empty(N, dtype=torch.int32, device="cuda")
    d_lcp = torch.empty(N, dtype=torch.int32, device="cuda")
    pt, psa, pl = (C.c_void_p(t.data_ptr()) for t in (d_text, d_sa, d_lcp))
    assert lib.tc_generate_dev(h, kind, 0xC2, n, pt) == 0
    torch.cuda.synchronize()
    sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(h, pt, n, psa)))
    lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(h, pt, n, psa, pl)))
    mx, row, tot = C.c_uint32(), C.c_uint64(), C.c_uint64()
    floor_ms = timed(lambda: ctx._check(lib.tc_lcp_summary_dev(h, pl, N, C.byref(mx), C.byref(row), C.byref(tot))))
    name = NAMES.get(kind, str(kind))

    def line(call, ms, nbytes, count):
        print("%-13s | %2d | %-28s | %8.3f | %6.2f | %9.1f | %7.1f | %10d"
              % (name, log2, call, ms, ms / floor_ms, nbytes / 1e6, nbytes / ms / 1e6, count), flush=True)

    line("sort (tc_suffix_array_dev)", sort_ms, 0, 0)
    line("lcp (tc_lcp_array_dev)", lcp_ms, 0, 0)
    line("floor (tc_lcp_summary_dev)", floor_ms, 4 * N, int(mx.value))
    for k in a.k:
        groups = 0
        for mn, mo in ((1, 0), (2, 0)):
            nk = C.c_uint64(0)

            def count():
                nk.value = 0
                ctx._check(lib.tc_kmers_esa_dev(h, psa, pl, N, k, mn, mo, None, None, None, C.byref(nk)))
            count_ms = timed(count)
            z = int(nk.value)
            if (mn, mo) == (1, 0):
                groups = z
            outs = [torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            po = [C.c_void_p(o.data_ptr()) for o in outs]

            def full():
                nk.value = max(z, 1)
                ctx._check(lib.tc_kmers_esa_dev(h, psa, pl, N, k, mn, mo, po[0], po[1], po[2], C.byref(nk)))
            full_ms = timed(full)
            assert int(nk.value) == z
            line("list k=%d (%d,%d) sizes-only" % (k, mn, mo), count_ms, 8 * N + 4 * groups, z)
            line("list k=%d (%d,%d)" % (k, mn, mo), full_ms, 12 * N + 8 * groups + 12 * z, z)
            del outs
        d_hist = torch.empty(a.bins, dtype=torch.int64, device="cuda")
        dist, total = C.c_uint64(), C.c_uint64()
        ms = timed(lambda: ctx._check(lib.tc_kmer_spectrum_esa_dev(h, psa, pl, N, k, a.bins, C.c_void_p(d_hist.data_ptr()),
                                                                   C.byref(dist), C.byref(total))))
        assert int(dist.value) == groups
        line("spectrum k=%d bins=%d" % (k, a.bins), ms, 8 * N + 4 * groups, int(dist.value))
    import numpy as np
    d, u = np.zeros(a.kmax, np.uint64), np.zeros(a.kmax, np.uint64)
    ms = timed(lambda: ctx._check(lib.tc_kmer_profile_esa_dev(h, pl, N, a.kmax, C.c_void_p(d.ctypes.data), C.c_void_p(u.ctypes.data))))
    line("profile kmax=%d" % a.kmax, ms, 4 * N, int(d[min(a.kmax, 21) - 1]))
    # yardstick b: what the repeats add over their ESA
    nrep = C.c_uint64(0)
    ctx._check(lib.tc_repeats_dev(h, pt, n, 0, 1, 2, None, None, None, None, None, C.byref(nrep)))
    z = int(nrep.value)
    outs = [torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    po = [C.c_void_p(o.data_ptr()) for o in outs]

    def rep():
        nrep.value = max(z, 1)
        ctx._check(lib.tc_repeats_dev(h, pt, n, 0, 1, 2, None, po[0], po[1], po[2], po[3], C.byref(nrep)))
    rep_ms = timed(rep)
    line("rep+ (tc_repeats_dev - ESA)", rep_ms - sort_ms - lcp_ms, 0, z)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 2, 3, 4, 5, 6])
    ap.add_argument("--log2", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--k", type=int, nargs="+", default=[12, 21, 31])
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--kmax", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds one class and size may take")
    ap.add_argument("--child", type=int, nargs=2, metavar=("KIND", "LOG2"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, *a.child)
        return 0
    print(HEADER, flush=True)
    for log2 in a.log2:
        for kind in a.kinds:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(kind), str(log2), "--bins", str(a.bins), "--kmax", str(a.kmax),
                   "--steps", str(a.steps), "--warmup", str(a.warmup), "--k"] + [str(k) for k in a.k]
            try:
                rc = subprocess.run(cmd, timeout=a.limit).returncode
            except subprocess.TimeoutExpired:
                print("# class %d at 2^%d ran into its limit of %d s: stopping" % (kind, log2, a.limit), flush=True)
                return 1
            if rc != 0:
                print("# class %d at 2^%d ended with status %d: stopping" % (kind, log2, rc), flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
