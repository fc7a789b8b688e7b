#!/usr/bin/env python3
"""The runs (tandem repeats) of a text on the device: tc_tandem_repeats_dev, per input class and size.

  python scripts/tandem_bench.py                        # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes
  python scripts/tandem_bench.py --kinds 0 --log2 26 --max-period 0 64

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/rep_bench.py).  Times are
HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup`
calls, then the median of `--steps` timed ones.  tc_tandem_repeats_dev is one call; what it adds is told apart by the calls
that stop earlier, on the same text and on its reverse, in the same run:
  ESA      tc_suffix_array_dev + tc_lcp_array_dev of the text
  ESA rev  the same of the reversed text (torch.flip): the call builds both
  added    the full tc_tandem_repeats_dev at its exact capacity - ESA - ESA rev  (the reversal, the two scatters, four trees,
           tr_cand_kernel, count, scan, fill, order)
  REP      tc_repeats_dev (maximal, min_len 1) at its exact capacity - ESA: what the maximal repeats add to one ESA
One line per class, size and max_period: the sizes-only call, the full call, added, added / (ESA + ESA rev), added / REP and
the number of runs."""
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
    ap.add_argument("--max-period", type=int, nargs="+", default=[0])
    ap.add_argument("--min-period", type=int, default=1)
    ap.add_argument("--min-copies", type=int, default=2)
    ap.add_argument("--min-len", type=int, default=1)
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

    print("# class | log2 n | sort ms | lcp ms | sort rev ms | lcp rev ms | repeats_dev (max, 1) ms | max_period | tandem sizes-only ms | tandem ms | added = tandem - ESA - ESA rev | added / both ESAs | REP = repeats_dev - ESA | added / REP | runs")
    for log2 in a.log2:
        n = 1 << log2
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_a = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_b = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        pt, pa, pb = (C.c_void_p(t.data_ptr()) for t in (d_text, d_a, d_b))
        for kind in a.kinds:
            assert lib.tc_generate_dev(ctx.handle, kind, 0xC2, n, pt) == 0
            torch.cuda.synchronize()
            d_rev = torch.flip(d_text, [0]).contiguous()
            torch.cuda.synchronize()
            pr = C.c_void_p(d_rev.data_ptr())
            sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, pt, n, pa)))
            lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, pt, n, pa, pb)))
            rsort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, pr, n, pa)))
            rlcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, pr, n, pa, pb)))
            del d_rev
            esa, both = sort_ms + lcp_ms, sort_ms + lcp_ms + rsort_ms + rlcp_ms
            nrep = C.c_uint64(0)
            ctx._check(lib.tc_repeats_dev(ctx.handle, pt, n, 0, 1, 2, None, None, None, None, None, C.byref(nrep)))
            zr = int(nrep.value)
            outs = [torch.empty(max(zr, 1), dtype=torch.int32, device="cuda") for _ in range(4)]
            torch.cuda.synchronize()
            po = [C.c_void_p(o.data_ptr()) for o in outs]

            def repeats():
                nrep.value = max(zr, 1)
                ctx._check(lib.tc_repeats_dev(ctx.handle, pt, n, 0, 1, 2, None, po[0], po[1], po[2], po[3], C.byref(nrep)))
            rep_ms = timed(repeats)
            del outs
            for max_period in a.max_period:
                nrun = C.c_uint64(0)
                f = (a.min_period, max_period, a.min_copies, a.min_len)

                def count():
                    nrun.value = 0
                    ctx._check(lib.tc_tandem_repeats_dev(ctx.handle, pt, n, *f, None, None, None, C.byref(nrun)))
                count_ms = timed(count)
                z = int(nrun.value)
                outs = [torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
                torch.cuda.synchronize()
                po = [C.c_void_p(o.data_ptr()) for o in outs]

                def full():
                    nrun.value = max(z, 1)
                    ctx._check(lib.tc_tandem_repeats_dev(ctx.handle, pt, n, *f, po[0], po[1], po[2], C.byref(nrun)))
                full_ms = timed(full)
                assert int(nrun.value) == z
                added = full_ms - both
                print("%-13s | %2d | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f | %5d | %8.3f | %8.3f | %8.3f | %6.3f | %8.3f | %6.3f | %10d"
                      % (NAMES.get(kind, str(kind)), log2, sort_ms, lcp_ms, rsort_ms, rlcp_ms, rep_ms, max_period, count_ms, full_ms,
                         added, added / both, rep_ms - esa, added / (rep_ms - esa), z), flush=True)
                del outs
        del d_text, d_a, d_b


if __name__ == "__main__":
    main()
