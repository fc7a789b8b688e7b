#!/usr/bin/env python3
"""The kept enhanced suffix array, on the device: tc_esa_build_dev and the batched queries tc_esa_lce_dev, tc_esa_find_dev and
tc_esa_compare_dev, per input class.

  python scripts/esa_bench.py                           # classes 0 2 4 5 at 2^28 bytes, 10^7 queries
  python scripts/esa_bench.py --kinds 0 --log2 26 --queries 1000000

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/cover_bench.py).  Times are HIP
events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained: `--warmup` calls, then
the median of `--steps` timed ones; every timed query batch is drawn afresh, so no call finds its lines cached by the one before.
Per class:
  build    tc_esa_build_dev + tc_esa_free against ESA = tc_suffix_array_dev + tc_lcp_array_dev into the caller's arrays: the
           difference is the copy of the text, the isa scatter, the two trees and six hipMalloc / hipFree
  lce      random pairs of positions at max_mismatch 0, 1, 4, 16: ms, queries per second, and the dependent random 64-byte lines
           the MODEL assumes per query -- at max_mismatch 0 the direct bytes of both positions, 2 lines, since on a random pair the
           first bytes decide -- as a fraction of the 53 G lines/s random-read wall of profiles/r03_fm_sweep.txt (50-56 G
           lines/s); the further turns of a larger max_mismatch mostly stay in those two lines
  find     random substrings of --find-len bytes without first_pos (MODEL: 2 lines: isa[start] and the line of lcp that holds the
           row and its successor -- a substring that occurs once ends both searches there) and with it
  compare  random pairs of substrings of --find-len bytes
  fm       find (occ only) on substrings of 20, 100 and 1000 bytes cut from the text against tc_fm_count_dev on the same substrings
           as patterns, on an index tc_fm_build_dev made in the same process; the counts must be equal
  kmers    ESAHandle.kmers(21) on the handle against Context.kmers_dev(text, 21), both at their exact capacity"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))

NAMES = {0: "iid ACGTN", 1: "ascii96", 2: "genome-like", 3: "zipf words", 4: "runs", 5: "period 4096", 6: "assembly gaps"}
WALL = 53e9     # random 64-byte lines per second: profiles/r03_fm_sweep.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 2, 4, 5])
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--queries", type=int, default=10 ** 7)
    ap.add_argument("--find-len", type=int, default=32)
    ap.add_argument("--fm-bytes", type=int, default=10 ** 8, help="pattern bytes of one batch of the comparison with tc_fm_count_dev")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-fm", action="store_true")
    a = ap.parse_args()
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib, h = ctx.lib, ctx.handle
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(h))
    n, nq = 1 << a.log2, a.queries

    def timed(fn, steps=a.steps, prep=None):
        ms = []
        for i in range(a.warmup + steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if prep:
                prep()      # fresh queries for every call: a repeated batch would find its lines in the last-level cache
            torch.cuda.synchronize()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def p(t):
        return C.c_void_p(t.data_ptr())

    def rand(hi, count):
        return torch.randint(0, hi, (count,), dtype=torch.int64, device="cuda").to(torch.int32)

    def rate(what, ms, count, lines=None):
        qps = count / (ms * 1e-3)
        model = "" if lines is None else " | model %d lines/query = %5.1f%% of the wall" % (lines, 100.0 * qps * lines / WALL)
        print("%-13s | %2d | %-28s | %9.3f ms | %8.1f M queries/s%s" % (name, a.log2, what, ms, qps / 1e6, model), flush=True)

    torch.manual_seed(0xE5A)
    for kind in a.kinds:
        name = NAMES.get(kind, str(kind))
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        pt = p(d_text)
        assert lib.tc_generate_dev(h, kind, 0xC2, n, pt) == 0
        d_sa, d_lcp = (torch.empty(n + 1, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        sort_ms = timed(lambda: ctx._check(lib.tc_suffix_array_dev(h, pt, n, p(d_sa))))
        lcp_ms = timed(lambda: ctx._check(lib.tc_lcp_array_dev(h, pt, n, p(d_sa), p(d_lcp))))
        del d_sa, d_lcp

        def build():
            hh = C.c_void_p()
            ctx._check(lib.tc_esa_build_dev(h, pt, n, C.byref(hh)))
            lib.tc_esa_free(hh)
        build_ms = timed(build)
        esa = sort_ms + lcp_ms
        print("%-13s | %2d | build %9.3f ms | sort %9.3f + lcp %9.3f = ESA %9.3f ms | build - ESA %8.3f ms = %5.1f%% of ESA"
              % (name, a.log2, build_ms, sort_ms, lcp_ms, esa, build_ms - esa, 100.0 * (build_ms - esa) / esa), flush=True)
        H = ctx.esa_build_dev(d_text)
        print("%-13s | %2d | handle: %d bytes = %.3f per text byte (text %d, sa %d, isa %d, lcp + tree %d, sa tree %d)"
              % ((name, a.log2, H.device_bytes(0), H.device_bytes(0) / n) + tuple(H.device_bytes(k) for k in range(1, 6))), flush=True)
        eh = H._h
        # ---- lce
        qa, qb = rand(n + 1, nq), rand(n + 1, nq)
        out = [torch.empty(nq, dtype=torch.int32, device="cuda") for _ in range(3)]
        for m in (0, 1, 4, 16):
            ms = timed(lambda: ctx._check(lib.tc_esa_lce_dev(h, eh, p(qa), p(qb), nq, m, p(out[0]), p(out[1]))),
                       prep=lambda: (qa.random_(0, n + 1), qb.random_(0, n + 1)))
            rate("lce max_mismatch %2d" % m, ms, nq, 2 if m == 0 else None)
            print("%-13s | %2d |   mean len %.2f, mean mismatches %.2f" % (name, a.log2, out[0].double().mean().item(), out[1].double().mean().item()), flush=True)
        # ---- find, compare
        L = a.find_len
        qs, ql = rand(n - L, nq), torch.full((nq,), L, dtype=torch.int32, device="cuda")
        fresh = lambda: qs.random_(0, n - L)
        ms = timed(lambda: ctx._check(lib.tc_esa_find_dev(h, eh, p(qs), p(ql), nq, p(out[0]), p(out[1]), None)), prep=fresh)
        rate("find len %d, no first_pos" % L, ms, nq, 2)
        print("%-13s | %2d |   mean occ %.2f, %.1f%% occur once" % (name, a.log2, out[1].double().mean().item(), 100.0 * (out[1] == 1).double().mean().item()), flush=True)
        ms = timed(lambda: ctx._check(lib.tc_esa_find_dev(h, eh, p(qs), p(ql), nq, p(out[0]), p(out[1]), p(out[2]))), prep=fresh)
        rate("find len %d, first_pos" % L, ms, nq)
        qs2 = rand(n - L, nq)
        order = torch.empty(nq, dtype=torch.int8, device="cuda")
        ms = timed(lambda: ctx._check(lib.tc_esa_compare_dev(h, eh, p(qs), p(ql), p(qs2), p(ql), nq, p(order), p(out[0]))),
                   prep=lambda: (fresh(), qs2.random_(0, n - L)))
        rate("compare len %d" % L, ms, nq)
        del qa, qb, qs2, order
        # ---- find against the FM-index on the same substrings
        if not a.no_fm:
            fm = ctx.fm_build_dev(d_text)
            for L in (20, 100, 1000):
                cnt = max(a.fm_bytes // L, 1)
                s = rand(n - L, cnt)
                ln = torch.full((cnt,), L, dtype=torch.int32, device="cuda")
                pats = d_text[(s.to(torch.int64)[:, None] + torch.arange(L, device="cuda")[None, :]).reshape(-1)].contiguous()
                offs = torch.arange(cnt + 1, dtype=torch.int64, device="cuda") * L
                occ = torch.empty(cnt, dtype=torch.int32, device="cuda")
                fmc = torch.empty(cnt, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                find_ms = timed(lambda: ctx._check(lib.tc_esa_find_dev(h, eh, p(s), p(ln), cnt, None, p(occ), None)))
                fm_ms = timed(lambda: ctx._check(lib.tc_fm_count_dev(h, fm._h, p(pats), p(offs), cnt, p(fmc))))
                assert torch.equal(occ.to(torch.int64), fmc), "find and tc_fm_count_dev disagree"
                print("%-13s | %2d | %8d substrings of %4d bytes | find %9.3f ms | tc_fm_count_dev %9.3f ms | x %7.2f | counts equal"
                      % (name, a.log2, cnt, L, find_ms, fm_ms, fm_ms / find_ms), flush=True)
                del s, ln, pats, offs, occ, fmc
            fm.close()
        # ---- a second analysis on the handle
        k = 21
        got = H.kmers(k)
        cap = got[0].numel()
        del got
        on_handle = timed(lambda: H.kmers(k, cap=cap), steps=3)
        from_text = timed(lambda: ctx.kmers_dev(d_text, k, cap=cap), steps=3)
        print("%-13s | %2d | kmers k = %d, %d of them | on the handle %9.3f ms | kmers_dev from the text %9.3f ms | x %6.2f"
              % (name, a.log2, k, cap, on_handle, from_text, from_text / on_handle), flush=True)
        H.close()
        del out, qs, ql, d_text


if __name__ == "__main__":
    main()
