#!/usr/bin/env python3
"""What is unique in a text, on the device: tc_unique_prefixes_dev, tc_unique_substrings_dev and tc_shortest_unique_dev, per
input class and size.

  python scripts/sus_bench.py                         # classes 0 2 4 5 at 2^26 and 2^28 bytes
  python scripts/sus_bench.py --kinds 0 --log2 26

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/maw_bench.py).  Times are
HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup`
calls, then the median of `--steps` timed ones.  What a call adds is told apart by the calls that stop earlier on the same
text in the same run:
  ESA      tc_suffix_array_dev + tc_lcp_array_dev (the sort and the LCP array: the yardstick)
  REP      tc_repeats_dev (maximal, min_len 1) at its exact capacity - ESA   (the project's yardstick for an ESA application)
  added    the call - ESA: sus_prefix_kernel for the prefixes (so n / added is that kernel's rate in rows/s); that, the count
           pass, the scan and the fill pass for the list at its exact capacity; the prefix and mark passes, the two scans, the
           tree and sus_point_kernel for the point call
One line per class, size and call: the call, added, added / ESA, added / REP, and the number of MUS."""
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
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 2, 4, 5])
    ap.add_argument("--log2", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-repeats", action="store_true", help="skip the tc_repeats_dev yardstick")
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

    print("# class | log2 n | sort ms | lcp ms | repeats_dev ms | REP = repeats - ESA | call | call ms | added = call - ESA | added / ESA | added / REP | G positions/s of added | MUS")
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
            esa = sort_ms + lcp_ms
            rep_ms = rep = float("nan")
            if not a.no_repeats:
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
                rep = rep_ms - esa
            head = "%-13s | %2d | %8.3f | %8.3f | %8.3f | %8.3f" % (NAMES.get(kind, str(kind)), log2, sort_ms, lcp_ms, rep_ms, rep)

            def line(what, ms, z):
                added = ms - esa
                print("%s | %-8s | %8.3f | %8.3f | %6.3f | %6.3f | %7.2f | %12d"
                      % (head, what, ms, added, added / esa, added / rep, n / added / 1e6 if added > 0 else float("nan"), z), flush=True)

            nmus = C.c_uint64(0)
            ctx._check(lib.tc_unique_substrings_dev(ctx.handle, pt, n, 1, 0, None, None, C.byref(nmus)))
            z = int(nmus.value)
            line("prefixes", timed(lambda: ctx._check(lib.tc_unique_prefixes_dev(ctx.handle, pt, n, pa))), z)
            start, ln = (torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            pw = [C.c_void_p(o.data_ptr()) for o in (start, ln)]

            def full():
                nmus.value = max(z, 1)
                ctx._check(lib.tc_unique_substrings_dev(ctx.handle, pt, n, 1, 0, pw[0], pw[1], C.byref(nmus)))
            line("list", timed(full), z)
            assert int(nmus.value) == z
            del start, ln
            line("point", timed(lambda: ctx._check(lib.tc_shortest_unique_dev(ctx.handle, pt, n, pa, pb))), z)
        del d_text, d_a, d_b


if __name__ == "__main__":
    main()
