#!/usr/bin/env python3
"""The repeat cover of a text, on the device: tc_repeat_spans_dev, tc_repeat_mask_dev, tc_repeat_dedup_dev and the general form
tc_cover_*_dev, per input class and size.

  python scripts/cover_bench.py                         # classes 0 2 4 5 at 2^26 and 2^28 bytes
  python scripts/cover_bench.py --kinds 0 --log2 26

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/sus_bench.py).  Times are HIP
events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup` calls,
then the median of `--steps` timed ones.  What a call adds is told apart by the calls that stop earlier on the same text in the
same run:
  ESA      tc_suffix_array_dev + tc_lcp_array_dev (the sort and the LCP array: the yardstick)
  REP      tc_repeats_dev (maximal, min_len 1) at its exact capacity - ESA
  MUS      tc_unique_substrings_dev (window (1, 0)) at its exact capacity - ESA
  added    the call - ESA: the zeroing of len, the trees where the call searches, cov_seed_kernel and the cover passes
One line per class, size, (min_len, min_occ, kind) and call: the call, added, added / ESA, added / MUS, added / REP, the spans and
the covered bytes.  Then the general form alone over the text's LPF array kept in HBM (tc_lpf_array_dev, not timed), beside one
plain read of that array (a sum over it on the same stream)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))

NAMES = {0: "iid ACGTN", 1: "ascii96", 2: "genome-like", 3: "zipf words", 4: "runs", 5: "period 4096", 6: "assembly gaps"}
CONFIGS = ((20, 2, 0), (20, 2, 1), (12, 10, 0))     # (min_len, min_occ, kind)
KIND = ("ALL", "LATER")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 2, 4, 5])
    ap.add_argument("--log2", type=int, nargs="+", default=[26, 28])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-yardsticks", action="store_true", help="skip tc_repeats_dev and tc_unique_substrings_dev")
    a = ap.parse_args()
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib, h = ctx.lib, ctx.handle
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(h))

    def timed(fn, on=stream):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(on)
            fn()
            e1.record(on)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    soft = textcomp.SOFT_MASK.copy()
    pm = soft.ctypes.data_as(C.c_void_p)
    print("# class | log2 n | sort ms | lcp ms | REP = repeats - ESA | MUS = unique_substrings - ESA | L q kind | call | call ms | added = call - ESA | added / ESA | added / MUS | added / REP | spans | covered")
    for log2 in a.log2:
        n = 1 << log2
        d_text, d_out = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_a = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_b = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        pt, po, pa, pb = (C.c_void_p(t.data_ptr()) for t in (d_text, d_out, d_a, d_b))
        for kind in a.kinds:
            assert lib.tc_generate_dev(h, kind, 0xC2, n, pt) == 0
            torch.cuda.synchronize()
            sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(h, pt, n, pa)))
            lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(h, pt, n, pa, pb)))
            esa = sort_ms + lcp_ms
            rep = mus = float("nan")
            if not a.no_yardsticks:
                cnt = C.c_uint64(0)
                ctx._check(lib.tc_repeats_dev(h, pt, n, 0, 1, 2, None, None, None, None, None, C.byref(cnt)))
                z = max(int(cnt.value), 1)
                outs = [torch.empty(z, dtype=torch.int32, device="cuda") for _ in range(4)]
                torch.cuda.synchronize()
                pz = [C.c_void_p(o.data_ptr()) for o in outs]

                def repeats():
                    cnt.value = z
                    ctx._check(lib.tc_repeats_dev(h, pt, n, 0, 1, 2, None, pz[0], pz[1], pz[2], pz[3], C.byref(cnt)))
                rep = timed(repeats) - esa
                del outs
                cnt.value = 0
                ctx._check(lib.tc_unique_substrings_dev(h, pt, n, 1, 0, None, None, C.byref(cnt)))
                z = max(int(cnt.value), 1)
                outs = [torch.empty(z, dtype=torch.int32, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()
                pz = [C.c_void_p(o.data_ptr()) for o in outs]

                def unique():
                    cnt.value = z
                    ctx._check(lib.tc_unique_substrings_dev(h, pt, n, 1, 0, pz[0], pz[1], C.byref(cnt)))
                mus = timed(unique) - esa
                del outs
            head = "%-13s | %2d | %8.3f | %8.3f | %8.3f | %8.3f" % (NAMES.get(kind, str(kind)), log2, sort_ms, lcp_ms, rep, mus)

            def line(cfg, what, ms, base, spans, covered):
                added = ms - base
                print("%s | %-11s | %-6s | %8.3f | %8.3f | %6.3f | %6.3f | %6.3f | %11d | %11d"
                      % (head, cfg, what, ms, added, added / esa, added / mus, added / rep, spans, covered), flush=True)

            ns, nout, cov = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            for L, q, k in CONFIGS:
                cfg = "%d %d %s" % (L, q, KIND[k])
                ns.value = 0
                ctx._check(lib.tc_repeat_spans_dev(h, pt, n, L, q, k, None, None, C.byref(ns), C.byref(cov)))
                z, covered = int(ns.value), int(cov.value)
                start, ln = (torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(2))
                torch.cuda.synchronize()
                pw = [C.c_void_p(o.data_ptr()) for o in (start, ln)]

                def spans():
                    ns.value = max(z, 1)
                    ctx._check(lib.tc_repeat_spans_dev(h, pt, n, L, q, k, pw[0], pw[1], C.byref(ns), C.byref(cov)))
                line(cfg, "spans", timed(spans), esa, z, covered)
                assert (int(ns.value), int(cov.value)) == (z, covered)
                del start, ln
                line(cfg, "mask", timed(lambda: ctx._check(lib.tc_repeat_mask_dev(h, pt, n, L, q, k, pm, po, C.byref(cov)))), esa, z, covered)

                def dedup():
                    nout.value = n
                    ctx._check(lib.tc_repeat_dedup_dev(h, pt, n, L, q, k, po, C.byref(nout), C.byref(cov)))
                line(cfg, "dedup", timed(dedup), esa, z, covered)
                assert int(nout.value) == n - covered
            # the general form alone, over the LPF array kept in HBM (d_b), beside one plain read of it
            ctx._check(lib.tc_lpf_array_dev(h, pt, n, pb, None))
            torch.cuda.synchronize()
            d_lpf = d_b[:n]
            read_ms = timed(lambda: d_lpf.sum(dtype=torch.int64), on=torch.cuda.current_stream())
            L = 20
            ns.value = 0
            ctx._check(lib.tc_cover_spans_dev(h, pb, n, L, None, None, C.byref(ns), C.byref(cov)))
            z, covered = int(ns.value), int(cov.value)
            start, ln = (torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            pw = [C.c_void_p(o.data_ptr()) for o in (start, ln)]

            def gspans():
                ns.value = max(z, 1)
                ctx._check(lib.tc_cover_spans_dev(h, pb, n, L, pw[0], pw[1], C.byref(ns), C.byref(cov)))

            def gdedup():
                nout.value = n
                ctx._check(lib.tc_cover_dedup_dev(h, pb, pt, n, L, po, C.byref(nout), C.byref(cov)))
            for what, fn in (("spans", gspans), ("mask", lambda: ctx._check(lib.tc_cover_mask_dev(h, pb, pt, n, L, pm, po, C.byref(cov)))),
                             ("dedup", gdedup)):
                ms = timed(fn)
                print("%-13s | %2d | general form over lpf, L = %d | %-6s | %8.3f ms | one plain read of the array %8.3f ms | x %6.2f | %11d | %11d"
                      % (NAMES.get(kind, str(kind)), log2, L, what, ms, read_ms, ms / read_ms, z, covered), flush=True)
            del start, ln, d_lpf
        del d_text, d_out, d_a, d_b


if __name__ == "__main__":
    main()
