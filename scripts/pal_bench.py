#!/usr/bin/env python3
"""The palindromes / inverted repeats of a text on the device: tc_palindromes_dev, per input class, size and budget.

  python scripts/pal_bench.py                           # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes, m = 0 1 4 16
  python scripts/pal_bench.py --kinds 0 --log2 26 --mismatch 0 --identity

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/rep_bench.py).  Times are
HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup`
calls, then the median of `--steps` timed ones.  tc_palindromes_dev is one call; what it adds is told apart by the calls
that stop earlier, on the joint text S = text . sigma(reverse(text)) of 2n bytes (built here with torch), in the same run:
  ESA(S)   tc_suffix_array_dev + tc_lcp_array_dev of S
  added    the full tc_palindromes_dev at its exact capacity - ESA(S)  (the joint text, the scatter, one tree,
           pal_centre_kernel, count, scan, fill)
  fill     the full call - the sizes-only call
  TR       tc_tandem_repeats_dev at its exact capacity - the ESAs of the text and of its reverse: what the runs add, the
           yardstick at m = 0 (--no-tandem leaves it out)
  longest  tc_longest_palindrome_dev
sigma is the DNA complement (--identity: the identity).  One line per class, size and budget."""
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
    ap.add_argument("--mismatch", type=int, nargs="+", default=[0, 1, 4, 16])
    ap.add_argument("--min-len", type=int, default=8)
    ap.add_argument("--identity", action="store_true")
    ap.add_argument("--no-tandem", action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import numpy as np
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(ctx.handle))
    comp = None if a.identity else np.ascontiguousarray(textcomp.DNA_COMPLEMENT)
    pcomp = comp.ctypes.data_as(C.c_void_p) if comp is not None else None

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

    print("# sigma: %s, min_len %d" % ("identity" if a.identity else "DNA complement", a.min_len))
    print("# class | log2 n | sort(S) ms | lcp(S) ms | TR = tandem - its two ESAs ms | m | sizes-only ms | full ms | added = full - ESA(S) | added / ESA(S) | fill | added / TR | centres/s of the added time | longest ms | palindromes | longest (start, len, mm)")
    for log2 in a.log2:
        n = 1 << log2
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        pt = C.c_void_p(d_text.data_ptr())
        for kind in a.kinds:
            assert lib.tc_generate_dev(ctx.handle, kind, 0xC2, n, pt) == 0
            torch.cuda.synchronize()
            d_a = torch.empty(2 * n + 1, dtype=torch.int32, device="cuda")
            d_b = torch.empty(2 * n + 1, dtype=torch.int32, device="cuda")
            pa, pb = C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr())
            d_rev = torch.flip(d_text, [0]).contiguous()
            tr_ms = float("nan")
            if not a.no_tandem:
                pr = C.c_void_p(d_rev.data_ptr())
                both = 0.0
                for p in (pt, pr):
                    both += timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, p, n, pa)))
                    both += timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, p, n, pa, pb)))
                nrun = C.c_uint64(0)
                ctx._check(lib.tc_tandem_repeats_dev(ctx.handle, pt, n, 1, 0, 2, 1, None, None, None, C.byref(nrun)))
                zr = int(nrun.value)
                outs = [torch.empty(max(zr, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
                torch.cuda.synchronize()
                po = [C.c_void_p(o.data_ptr()) for o in outs]

                def tandem():
                    nrun.value = max(zr, 1)
                    ctx._check(lib.tc_tandem_repeats_dev(ctx.handle, pt, n, 1, 0, 2, 1, po[0], po[1], po[2], C.byref(nrun)))
                tr_ms = timed(tandem) - both
                del outs
            if comp is not None:
                d_rev = torch.from_numpy(comp).cuda()[d_rev.long()]
            d_S = torch.cat((d_text, d_rev))
            del d_rev
            torch.cuda.synchronize()
            ps = C.c_void_p(d_S.data_ptr())
            sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, ps, 2 * n, pa)))
            lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, ps, 2 * n, pa, pb)))
            del d_S, d_a, d_b
            esa = sort_ms + lcp_ms
            for m in a.mismatch:
                npal = C.c_uint64(0)

                def count():
                    npal.value = 0
                    ctx._check(lib.tc_palindromes_dev(ctx.handle, pt, n, pcomp, m, a.min_len, None, None, None, C.byref(npal)))
                count_ms = timed(count)
                z = int(npal.value)
                outs = [torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
                torch.cuda.synchronize()
                po = [C.c_void_p(o.data_ptr()) for o in outs]

                def full():
                    npal.value = max(z, 1)
                    ctx._check(lib.tc_palindromes_dev(ctx.handle, pt, n, pcomp, m, a.min_len, po[0], po[1], po[2], C.byref(npal)))
                full_ms = timed(full)
                assert int(npal.value) == z
                del outs
                best = []
                long_ms = timed(lambda: best.append(ctx.longest_palindrome_dev(d_text, comp, m)))
                added = full_ms - esa
                print("%-13s | %2d | %8.3f | %8.3f | %8.3f | %2d | %8.3f | %8.3f | %8.3f | %6.3f | %7.3f | %6.3f | %6.2f G | %8.3f | %10d | %s"
                      % (NAMES.get(kind, str(kind)), log2, sort_ms, lcp_ms, tr_ms, m, count_ms, full_ms, added, added / esa,
                         full_ms - count_ms, added / tr_ms, (2 * n - 1) / added / 1e6, long_ms, z, best[-1]), flush=True)
        del d_text


if __name__ == "__main__":
    main()
