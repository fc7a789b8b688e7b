#!/usr/bin/env python3
"""The minimal absent words of a text on the device: tc_absent_words_dev and tc_absent_word_profile_dev, per input class and size.

  python scripts/maw_bench.py                         # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes, windows max_len 0 and 16
  python scripts/maw_bench.py --kinds 0 --log2 26 --max-len 16

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/rep_bench.py).  Times are
HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup`
calls, then the median of `--steps` timed ones.  What a call adds is told apart by the calls that stop earlier on the same
text in the same run:
  ESA      tc_suffix_array_dev + tc_lcp_array_dev (the sort and the LCP array: the yardstick)
  REP      tc_repeats_dev (maximal, min_len 1) at its exact capacity - ESA   (the nearest existing call: the same searches and
           change counts, one tree fewer, a fixed output)
  added    the full tc_absent_words_dev at its exact capacity - ESA   (the two trees, the change counts, the count pass, the
           scan, the fill pass), or tc_absent_word_profile_dev - ESA (one histogram pass instead of count, scan and fill)
One line per class, size and window: the sizes-only call, the full call, added, added / ESA, added / REP and the number of
words; one line per class and size for the profile."""
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
    ap.add_argument("--max-len", type=int, nargs="+", default=[0, 16])
    ap.add_argument("--kmax", type=int, default=64)
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

    print("# class | log2 n | sort ms | lcp ms | repeats_dev ms | REP = repeats - ESA | what | max_len | sizes-only ms | full ms | added = full - ESA | added / ESA | added / REP | words")
    for log2 in a.log2:
        n = 1 << log2
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_a = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_b = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_hist = torch.zeros(a.kmax + 1, dtype=torch.int64, device="cuda")
        pt, pa, pb, ph = (C.c_void_p(t.data_ptr()) for t in (d_text, d_a, d_b, d_hist))
        for kind in a.kinds:
            assert lib.tc_generate_dev(ctx.handle, kind, 0xC2, n, pt) == 0
            torch.cuda.synchronize()
            sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, pt, n, pa)))
            lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, pt, n, pa, pb)))
            esa = sort_ms + lcp_ms
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
            for max_len in a.max_len:
                nmaw = C.c_uint64(0)

                def count():
                    nmaw.value = 0
                    ctx._check(lib.tc_absent_words_dev(ctx.handle, pt, n, 2, max_len, None, None, None, C.byref(nmaw)))
                count_ms = timed(count)
                z = int(nmaw.value)
                left = torch.empty(max(z, 1), dtype=torch.uint8, device="cuda")
                pos, ln = (torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(2))
                torch.cuda.synchronize()
                pw = [C.c_void_p(o.data_ptr()) for o in (left, pos, ln)]

                def full():
                    nmaw.value = max(z, 1)
                    ctx._check(lib.tc_absent_words_dev(ctx.handle, pt, n, 2, max_len, pw[0], pw[1], pw[2], C.byref(nmaw)))
                full_ms = timed(full)
                assert int(nmaw.value) == z
                added = full_ms - esa
                print("%s | list    | %2d | %8.3f | %8.3f | %8.3f | %6.3f | %6.3f | %12d"
                      % (head, max_len, count_ms, full_ms, added, added / esa, added / rep, z), flush=True)
                del left, pos, ln
            total = C.c_uint64(0)
            prof_ms = timed(lambda: ctx._check(lib.tc_absent_word_profile_dev(ctx.handle, pt, n, a.kmax, ph, C.byref(total))))
            added = prof_ms - esa
            print("%s | profile | %2d | %8s | %8.3f | %8.3f | %6.3f | %6.3f | %12d"
                  % (head, a.kmax, "-", prof_ms, added, added / esa, added / rep, int(total.value)), flush=True)
        del d_text, d_a, d_b, d_hist


if __name__ == "__main__":
    main()
