#!/usr/bin/env python3
"""The LZ77 parse of a text against itself on the device: tc_lz_parse_dev and tc_lz_unparse_dev, per input class and size.

  python scripts/lz_bench.py                         # classes 0 2 3 4 5 6 at 2^26 and 2^28 bytes
  python scripts/lz_bench.py --kinds 0 --log2 26 --tile 16384

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/lcp_bench.py).  Times are
HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup`
calls, then the median of `--steps` timed ones.  tc_lz_parse_dev is one call; its parts are told apart by the calls that
stop earlier on the same text in the same run:
  ESA      tc_suffix_array_dev + tc_lcp_array_dev (the sort and the LCP array: the yardstick)
  LPF      tc_lpf_array_dev - ESA        (the two min trees, lz_lpf_kernel, and the pass that unpacks (lpf, src), which the
                                          parse does not run: about 12 bytes per text byte streamed)
  starts   the sizes-only tc_lz_parse_dev - tc_lpf_array_dev   (tile exits, the serial chain over the tiles, the marking
                                          and the scan; too small by that unpacking pass)
  fill     the full tc_lz_parse_dev - the sizes-only one
The ratio is (the full tc_lz_parse_dev - ESA) / ESA: what the parse adds to the enhanced suffix array it needs.  Then
tc_lz_unparse_dev of that parse at its exact capacity, checked against the text, and the phrase count z."""
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
    ap.add_argument("--tile", type=int, default=0, help="positions per tile of the phrase-start steps (0: the library's LZ_TILE)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(ctx.handle))
    lib.tc_dbg_lz_set_tile.argtypes = [C.c_void_p, C.c_uint32]
    assert lib.tc_dbg_lz_set_tile(ctx.handle, a.tile) == 0

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

    print("# class | log2 n | sort ms | lcp ms | lpf_array_dev ms | parse sizes-only ms | parse ms | = ESA + LPF + starts + fill | (parse - ESA) / ESA | unparse ms | phrases z | n / z")
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
            nph = C.c_uint64(0)

            def count():
                nph.value = 0
                ctx._check(lib.tc_lz_parse_dev(ctx.handle, pt, n, None, None, C.byref(nph)))
            count_ms = timed(count)
            z = int(nph.value)
            d_ps = torch.empty(z, dtype=torch.int32, device="cuda")
            d_pl = torch.empty(z, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ps, pl = C.c_void_p(d_ps.data_ptr()), C.c_void_p(d_pl.data_ptr())

            def parse():
                nph.value = z
                ctx._check(lib.tc_lz_parse_dev(ctx.handle, pt, n, ps, pl, C.byref(nph)))
            parse_ms = timed(parse)
            assert int(nph.value) == z
            d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            nb = C.c_uint64(0)

            def unparse():
                nb.value = n
                ctx._check(lib.tc_lz_unparse_dev(ctx.handle, ps, pl, z, C.c_void_p(d_out.data_ptr()), C.byref(nb)))
            un_ms = timed(unparse)
            assert int(nb.value) == n and bool(torch.equal(d_out, d_text)), "unparse(parse(text)) is not the text"
            esa = sort_ms + lcp_ms
            print("%-13s | %2d | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f | %8.3f + %7.3f + %7.3f + %7.3f | %6.3f | %8.3f | %10d | %.1f"
                  % (NAMES.get(kind, str(kind)), log2, sort_ms, lcp_ms, lpf_ms, count_ms, parse_ms, esa, lpf_ms - esa,
                     count_ms - lpf_ms, parse_ms - count_ms, (parse_ms - esa) / esa, un_ms, z, n / max(z, 1)), flush=True)
            del d_ps, d_pl, d_out
        del d_text, d_a, d_b


if __name__ == "__main__":
    main()
