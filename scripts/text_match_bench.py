#!/usr/bin/env python3
"""One text against another on the device: tc_text_match_stats_dev, tc_mems_from_stats_dev and the LCS pass, per input
class and size, beside the calls they are measured against.

  python scripts/text_match_bench.py                          # legs a, b and c at their default sizes
  python scripts/text_match_bench.py --legs a --kinds 0 --log2 25

Every (leg, class, size) runs in a child process of its own under `timeout` (--limit seconds), one after the other; the
first child that fails ends the run.  The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes
of scripts/lcp_bench.py): one text of a + b bytes, Q its first a bytes and T the rest.  Times are HIP events on the
context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup` calls, then the
median of `--steps` timed ones.

  leg a  a = b = 2^log2: what tc_text_match_stats_dev adds over the enhanced suffix array of the same n = a + b bytes
         (tc_suffix_array_dev + tc_lcp_array_dev of Q T), with all three arrays and with ms_len alone, and tc_text_lcs_dev, beside what
         tc_lpf_array_dev adds over that same ESA in the same run
  leg b  a = 2^20, b = 2^27: the same answer through tc_fm_match_stats_dev with Q as one pattern on tc_fm_build_lcp_dev(T)
         (the build is timed apart: an index serves many queries), and the two answers compared
  leg c  a = b = 2^log2: tc_mems_from_stats_dev, sizes-only and full, at min_len 1 and 20, against one plain read of the
         array (tc_lcp_summary_dev over ms_len, which is also the kernel of the LCS pass)"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))

NAMES = {0: "iid ACGTN", 1: "ascii96", 2: "genome-like", 3: "zipf words", 4: "runs", 5: "period 4096", 6: "assembly gaps"}


def one(a):
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib = ctx.lib
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(ctx.handle))

    def timed(fn, steps=a.steps):
        ms = []
        for i in range(a.warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    qa, tb = a.a, a.b
    n = qa + tb
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.tc_generate_dev(ctx.handle, a.kind, 0xC2, n, C.c_void_p(d_text.data_ptr())) == 0
    d_len, d_pos, d_occ = (torch.empty(qa, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    px, pq, pt = C.c_void_p(d_text.data_ptr()), C.c_void_p(d_text.data_ptr()), C.c_void_p(d_text.data_ptr() + qa)
    pl, pp, po = (C.c_void_p(t.data_ptr()) for t in (d_len, d_pos, d_occ))
    name = NAMES.get(a.kind, str(a.kind))

    def stats(pos=pp, occ=po):
        ctx._check(lib.tc_text_match_stats_dev(ctx.handle, pq, qa, pt, tb, pl, pos, occ))

    if a.leg == "a":
        d_a = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_b = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pa, pb = C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr())
        sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(ctx.handle, px, n, pa)))
        lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(ctx.handle, px, n, pa, pb)))
        lpf_ms = timed(lambda: ctx._check(lib.tc_lpf_array_dev(ctx.handle, px, n, pa, pb)))
        tm_ms = timed(stats)
        len_ms = timed(lambda: stats(None, None))
        best, qpos, tpos, tot = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        lcs_ms = timed(lambda: ctx._check(lib.tc_text_lcs_dev(ctx.handle, pq, qa, pt, tb, C.byref(best), C.byref(qpos), C.byref(tpos), C.byref(tot))))
        assert (best.value, tot.value) == (int(d_len.max()), int(d_len.long().sum()))
        esa = sort_ms + lcp_ms
        print("a | %-13s | a = b = 2^%d | sort %9.3f | lcp %9.3f | lpf_array_dev %9.3f (ESA + %8.3f) | text_match_stats_dev %9.3f (ESA + %8.3f)"
              " | ms_len alone %9.3f (ESA + %8.3f) | text_lcs_dev %9.3f (ESA + %8.3f) | added / LPF's added %.2f | mean ms_len %.1f"
              % (name, a.log2, sort_ms, lcp_ms, lpf_ms, lpf_ms - esa, tm_ms, tm_ms - esa, len_ms, len_ms - esa, lcs_ms, lcs_ms - esa,
                 (tm_ms - esa) / max(lpf_ms - esa, 1e-9), float(d_len.double().mean())), flush=True)
    elif a.leg == "b":
        tm_ms = timed(stats)
        d_t = d_text[qa:]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fm = ctx.fm_build_dev(d_t, lcp=True)
        e1.record(stream)
        e1.synchronize()
        build_ms = e0.elapsed_time(e1)
        d_offs = torch.tensor([0, qa], dtype=torch.int64, device="cuda")
        f_len = torch.zeros(qa, dtype=torch.int32, device="cuda")
        f_pos = torch.zeros(qa, dtype=torch.int64, device="cuda")
        f_occ = torch.zeros(qa, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def fm_stats():
            ctx._check(lib.tc_fm_match_stats_dev(ctx.handle, fm._h, pq, C.c_void_p(d_offs.data_ptr()), 1, C.c_void_p(f_len.data_ptr()),
                                                 C.c_void_p(f_pos.data_ptr()), C.c_void_p(f_occ.data_ptr())))
        fm_ms = timed(fm_stats, steps=min(a.steps, 3))
        same = bool(torch.equal(f_len, d_len)) and bool(torch.equal(f_occ, d_occ)) and bool(
            torch.equal(f_pos - (f_len > 0).long(), d_pos.long()))
        fm.close()
        assert same, "the two paths differ"
        print("b | %-13s | a = 2^%d b = 2^%d | text_match_stats_dev %9.3f | fm_build_lcp_dev(T) %9.3f | fm_match_stats_dev, Q one pattern %11.3f"
              " | fm query / text_match_stats_dev %.1f | answers equal" % (name, a.log2a, a.log2, tm_ms, build_ms, fm_ms, fm_ms / tm_ms), flush=True)
    else:
        stats()
        mx, row, tot = C.c_uint32(), C.c_uint64(), C.c_uint64()
        read_ms = timed(lambda: ctx._check(lib.tc_lcp_summary_dev(ctx.handle, pl, qa, C.byref(mx), C.byref(row), C.byref(tot))))
        out = []
        for min_len in (1, 20):
            nmem = C.c_uint64(0)

            def count():
                nmem.value = 0
                ctx._check(lib.tc_mems_from_stats_dev(ctx.handle, pl, pp, qa, min_len, None, None, None, C.byref(nmem)))
            count_ms = timed(count)
            z = int(nmem.value)
            d_m = [torch.empty(max(z, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()

            def fill():
                nmem.value = z
                ctx._check(lib.tc_mems_from_stats_dev(ctx.handle, pl, pp, qa, min_len, *(C.c_void_p(t.data_ptr()) for t in d_m), C.byref(nmem)))
            fill_ms = timed(fill)
            out.append("min_len %2d: %10d MEMs, sizes-only %8.3f (%.2f reads), full %8.3f (%.2f reads)"
                       % (min_len, z, count_ms, count_ms / read_ms, fill_ms, fill_ms / read_ms))
        print("c | %-13s | a = b = 2^%d | lcp_summary_dev over ms_len (the LCS pass) %8.3f | %s | LCS %d at %d, sum %d"
              % (name, a.log2, read_ms, " | ".join(out), mx.value, row.value, tot.value), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 2, 5])
    ap.add_argument("--log2", type=int, nargs="+", default=[25, 27], help="legs a and c: a = b = 2^log2; leg b: b = 2^27")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--one", nargs=5, metavar=("LEG", "KIND", "LOG2A", "LOG2B", "LOG2"), help="(a child of this script)")
    a = ap.parse_args()
    if a.one:
        a.leg, a.kind, a.log2a, a.log2 = a.one[0], int(a.one[1]), int(a.one[2]), int(a.one[4])
        a.a, a.b = 1 << int(a.one[2]), 1 << int(a.one[3])
        one(a)
        return
    print("# times in ms: the median of %d calls behind %d warm-up call(s)" % (a.steps, a.warmup), flush=True)
    for leg in a.legs:
        for log2 in ([27] if leg == "b" else a.log2):
            for kind in a.kinds:
                la = 20 if leg == "b" else log2
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup",
                       str(a.warmup), "--one", leg, str(kind), str(la), str(log2), str(log2)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:
                    print("# leg %s, class %d, 2^%d: exit status %d -- the run ends here" % (leg, kind, log2, rc), flush=True)
                    sys.exit(rc)


if __name__ == "__main__":
    main()
