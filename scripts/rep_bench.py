#!/usr/bin/env python3
"""The maximal and supermaximal repeats of a text on the device: tc_repeats_dev, per input class and size.

  python scripts/rep_bench.py                         # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes
  python scripts/rep_bench.py --kinds 0 --log2 26 --min-len 1 20

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/lcp_bench.py).  Times are
HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup`
calls, then the median of `--steps` timed ones.  tc_repeats_dev is one call; what it adds is told apart by the calls that
stop earlier on the same text in the same run:
  ESA      tc_suffix_array_dev + tc_lcp_array_dev (the sort and the LCP array: the yardstick)
  LPF      tc_lpf_array_dev - ESA        (what the LPF array adds to the same ESA: the figure to compare with)
  added    the full tc_repeats_dev at its exact capacity - ESA   (the tree, the change counts, rep_row_kernel, count, scan, fill)
One line per class, size, kind (max / super) and min_len: the sizes-only call, the full call, added, added / ESA, added / LPF
and the number of repeats."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))

NAMES = {0: "iid ACGTN", 1: "ascii96", 2: "genome-like", 3: "zipf words", 4: "runs", 5: "period 4096", 6: "assembly gaps"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 2, 3, 4, 5, 6])
    ap.add_argument("--log2", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--min-len", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--min-occ", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(ctx.handle))

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

    print("# class | log2 n | sort ms | lcp ms | lpf_array_dev ms | kind | min_len | repeats sizes-only ms | repeats ms | added = repeats - ESA | added / ESA | LPF = lpf_array_dev - ESA | added / LPF | repeats")
    for log2 in a.log2:
        n = 1 << log2
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_a = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_b = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        pt, pa, pb = (C.c_void_p(t.data_ptr()) for t in (d_text, d_a, d_b))
        for kind in a.kinds:
            assert lib.tc_generate_dev(ctx.handle, kind, 0xC2, n, pt) == 0
            torch.cuda.synchronize()
            sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, pt, n, pa)))
            lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, pt, n, pa, pb)))
            lpf_ms = timed(lambda: ctx._check(lib.tc_lpf_array_dev(ctx.handle, pt, n, pa, pb)))
            esa = sort_ms + lcp_ms
            for rk in (0, 1):
                for min_len in a.min_len:
                    nrep = C.c_uint64(0)

                    def count():
                        nrep.value = 0
                        ctx._check(lib.tc_repeats_dev(ctx.handle, pt, n, rk, min_len, a.min_occ, None, None, None, None, None, C.byref(nrep)))
                    count_ms = timed(count)
                    z = int(nrep.value)
                    outs = [torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(4)]
                    torch.cuda.synchronize()
                    po = [C.c_void_p(o.data_ptr()) for o in outs]

                    def full():
                        nrep.value = max(z, 1)
                        ctx._check(lib.tc_repeats_dev(ctx.handle, pt, n, rk, min_len, a.min_occ, None, po[0], po[1], po[2], po[3], C.byref(nrep)))
                    full_ms = timed(full)
                    assert int(nrep.value) == z
                    added = full_ms - esa
                    print("%-13s | %2d | %8.3f | %8.3f | %8.3f | %-5s | %2d | %8.3f | %8.3f | %8.3f | %6.3f | %8.3f | %6.3f | %10d"
                          % (NAMES.get(kind, str(kind)), log2, sort_ms, lcp_ms, lpf_ms, "super" if rk else "max", min_len, count_ms,
                             full_ms, added, added / esa, lpf_ms - esa, added / (lpf_ms - esa), z), flush=True)
                    del outs
        del d_text, d_a, d_b


if __name__ == "__main__":
    main()
