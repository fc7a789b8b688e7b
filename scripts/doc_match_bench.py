#!/usr/bin/env python3
"""Cross-document matches on the kept enhanced suffix array, on the device: tc_esa_doc_match_dev and tc_esa_doc_shared_dev, per input
class and number of documents, each against code the library had before them, in the same process.

  python scripts/doc_match_bench.py                      # classes 0 2 4 5 at 2^28 bytes, 1 / 256 / 65535 documents
  python scripts/doc_match_bench.py --kinds 0 --log2 26 --ndocs 256

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/esa_docs_bench.py), cut into documents
of equal size.  Times are HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has
drained: `--warmup` calls, then the median of `--steps` timed ones.  Per class and number of documents:
  (a) match   tc_esa_doc_match_dev, xl only and all three arrays, both kinds, clamped, against ONE tc_esa_doc_count_dev(limit 2) batch
              over all positions at the single length --find-len: without doc_match a caller binary-searches the length with about
              log2(n) such batches, so the ratio to one is stated and the old way costs about log2(n) times the batch
  (b) lce     tc_esa_lce_dev on as many random pairs as the text has positions: the random-read rate of DESIGN 4.15 (two reads of
              isa and one range minimum per query) beside the match's rows per second (two range minima and three scattered stores)
  (c) shared  tc_esa_doc_shared_dev (shared and longest) at --min-len against tc_esa_doc_match_dev (xl) + tc_cover_mask_dev without a
              map on the same lengths, which is what a caller had to run and then still sum per document"""
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
    ap.add_argument("--ndocs", type=int, nargs="+", default=[1, 256, 65535])
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--find-len", type=int, default=32)
    ap.add_argument("--min-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import numpy as np
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib, h = ctx.lib, ctx.handle
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(h))
    n, L = 1 << a.log2, a.find_len

    def timed(fn, prep=None):
        ms = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if prep:
                prep()
            torch.cuda.synchronize()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def p(t):
        return C.c_void_p(t.data_ptr())

    def line(text):
        print("%-13s | %2d | %s" % (name, a.log2, text), flush=True)

    torch.manual_seed(0xD0C6)
    for kind in a.kinds:
        name = NAMES.get(kind, str(kind))
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert lib.tc_generate_dev(h, kind, 0xC2, n, p(d_text)) == 0
        torch.cuda.synchronize()
        nq = n - L
        qs = torch.arange(nq, dtype=torch.int32, device="cuda")
        ql = torch.full((nq,), L, dtype=torch.int32, device="cuda")
        qa, qb = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        out = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        mask = torch.empty(n, dtype=torch.uint8, device="cuda")
        cov = C.c_uint64(0)
        for ndocs in a.ndocs:
            ds = (np.arange(ndocs + 1, dtype=np.uint64) * n // ndocs).astype(np.uint32)
            tag = "%5d docs" % ndocs
            H = ctx.esa_build_docs_dev(d_text, ds)
            eh = H._h
            shared = torch.empty(ndocs, dtype=torch.int64, device="cuda")
            longest = torch.empty(ndocs, dtype=torch.int32, device="cuda")
            cnt_ms, clo, chi = timed(lambda: ctx._check(lib.tc_esa_doc_count_dev(h, eh, p(qs), p(ql), nq, 2, p(out[0]), None)))
            two = (out[0][:nq] == 2).double().mean().item()
            line("%s | one doc_count limit 2 batch, len %d, all %d positions | %9.3f ms (%.3f .. %.3f) | %8.1f M positions/s | %.1f%% in two documents | the old way: about %d batches = %9.1f ms"
                 % (tag, L, nq, cnt_ms, clo, chi, nq / cnt_ms / 1e3, 100 * two, a.log2, a.log2 * cnt_ms))

            def fresh_pairs():
                qa.random_(0, n)
                qb.random_(0, n)
            lce_ms, llo, lhi = timed(lambda: ctx._check(lib.tc_esa_lce_dev(h, eh, p(qa), p(qb), n, 0, p(out[0]), None)), prep=fresh_pairs)
            line("%s | lce, %d random pairs                             | %9.3f ms (%.3f .. %.3f) | %8.1f M queries/s" % (tag, n, lce_ms, llo, lhi, n / lce_ms / 1e3))
            xl_ms = {}
            for k, kname in ((0, "OTHER"), (1, "EARLIER")):
                ms1, lo1, hi1 = timed(lambda: ctx._check(lib.tc_esa_doc_match_dev(h, eh, k, 1, p(out[0]), None, None)))
                mean = out[0].double().mean().item()
                ms3, lo3, hi3 = timed(lambda: ctx._check(lib.tc_esa_doc_match_dev(h, eh, k, 1, p(out[0]), p(out[1]), p(out[2]))))
                xl_ms[k] = ms1
                line("%s | doc_match %-7s xl only | %9.3f ms (%.3f .. %.3f) | %8.1f M rows/s | x %5.2f of one doc_count batch, x %5.2f of lce | all three %9.3f ms (%.3f .. %.3f) | mean xl %.2f"
                     % (tag, kname, ms1, lo1, hi1, n / ms1 / 1e3, ms1 / cnt_ms, ms1 / lce_ms, ms3, lo3, hi3, mean))
            for k, kname in ((0, "OTHER"), (1, "EARLIER")):
                sh_ms, slo, shi = timed(lambda: ctx._check(lib.tc_esa_doc_shared_dev(h, eh, k, a.min_len, p(shared), p(longest))))
                ctx._check(lib.tc_esa_doc_match_dev(h, eh, k, 1, p(out[0]), None, None))
                mk_ms, _, _ = timed(lambda: ctx._check(lib.tc_cover_mask_dev(h, p(out[0]), None, n, a.min_len, None, p(mask), C.byref(cov))))
                line("%s | doc_shared %-7s min_len %d | %9.3f ms (%.3f .. %.3f) | doc_match xl %9.3f ms + cover_mask %8.3f ms = %9.3f ms | x %5.2f | %d of %d bytes shared, longest %d"
                     % (tag, kname, a.min_len, sh_ms, slo, shi, xl_ms[k], mk_ms, xl_ms[k] + mk_ms, sh_ms / (xl_ms[k] + mk_ms),
                        int(shared.sum().item()), n, int(longest.max().item())))
                assert int(shared.sum().item()) == cov.value, (int(shared.sum().item()), cov.value)
            H.close()
            del shared, longest
        del d_text, qs, ql, qa, qb, out, mask


if __name__ == "__main__":
    main()
