#!/usr/bin/env python3
"""Suffix array and LCP array on the device: tc_suffix_array_dev, then tc_lcp_array_dev, per input class and size.

  python scripts/lcp_bench.py                         # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes
  python scripts/lcp_bench.py --kinds 0 2 5 --log2 26 --caps 64 256 1024      # the sweep of the short cap

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (kinds: 0 iid ACGTN, 2 genome-like, 3 Zipf words,
4 runs, 5 period 4096, 6 assembly with gaps).  Times are HIP events on the context's stream (tc_ctx_stream) around one
call, which returns after the stream has drained: `--warmup` calls, then the median of `--steps` timed ones.  The
yardstick is the sort itself: the LCP time stands next to the time tc_suffix_array_dev takes on the same text in the same
run.  The two streaming steps move 8 bytes per row coalesced and 4 bytes per row at random (the scatter writes, the gather
reads), so G rows/s of the whole call is a lower bound for their random-access rate.  --caps sets the short cap of
the one-lane compare kernel per run (tc_dbg_lcp_set_short_cap).  One line per class, size and cap; the summary's values go along as a checksum."""
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
    ap.add_argument("--caps", type=int, nargs="+", default=[0], help="short caps to run (0: the library's default)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    import textcomp
    from textcomp import _lib
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
        return statistics.median(ms), min(ms), max(ms)

    print("# class | log2 n | cap | suffix_array_dev ms (min .. max) | lcp_array_dev ms (min .. max) | lcp / sort | G rows/s of lcp | max lcp, row, sum")
    for log2 in a.log2:
        n = 1 << log2
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_sa = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_lcp = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        pt, ps, pl = (C.c_void_p(t.data_ptr()) for t in (d_text, d_sa, d_lcp))
        for kind in a.kinds:
            assert lib.tc_generate_dev(ctx.handle, kind, 0xC2, n, pt) == 0
            torch.cuda.synchronize()
            sa_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, pt, n, ps)))
            for cap in a.caps:
                assert lib.tc_dbg_lcp_set_short_cap(ctx.handle, C.c_uint32(cap)) == 0
                lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, pt, n, ps, pl)))
                mx, row, tot = ctx.lcp_summary_dev(d_lcp)
                print("%-13s | %2d | %4d | %9.3f (%9.3f .. %9.3f) | %9.3f (%9.3f .. %9.3f) | %6.3f | %6.2f | %d %d %d"
                      % (NAMES.get(kind, str(kind)), log2, cap or _lib.TC_LCP_SHORT_CAP, *sa_ms, *lcp_ms, lcp_ms[0] / sa_ms[0],
                         (n + 1) / lcp_ms[0] / 1e6, mx, row, tot), flush=True)
        del d_text, d_sa, d_lcp


if __name__ == "__main__":
    main()
