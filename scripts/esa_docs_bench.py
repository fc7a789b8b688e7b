#!/usr/bin/env python3
"""Document collections on the kept enhanced suffix array, on the device: tc_esa_build_docs_dev, tc_esa_doc_count_dev,
tc_esa_doc_list_dev, tc_esa_kmer_docs_dev and tc_esa_kmer_doc_spectrum_dev, per input class and number of documents, each against
code the library had before them, in the same process.

  python scripts/esa_docs_bench.py                      # classes 0 2 4 5 at 2^28 bytes, 1 / 256 / 65535 documents, 10^7 queries
  python scripts/esa_docs_bench.py --kinds 0 --log2 26 --ndocs 256 --queries 1000000
  python scripts/esa_docs_bench.py --find-only          # tc_esa_find_dev alone (no new symbol: the script runs on an older tree too)

The text of a class is tc_generate_dev(kind, seed 0xC2) resident in HBM (the classes of scripts/esa_bench.py), cut into documents of
equal size.  Times are HIP events on the context's stream (tc_ctx_stream) around one call, which returns after the stream has drained:
`--warmup` calls, then the median of `--steps` timed ones; every timed query batch is drawn afresh, so no call finds its lines cached
by the one before.  Per class and number of documents:
  build    tc_esa_build_docs_dev + tc_esa_free against tc_esa_build_dev + tc_esa_free: the difference is the document part.  MODEL:
           the bytes its passes must move per row -- da reads sa and writes da (8); a pass of the sort reads its keys twice (4 from da
           or 8 from the items, for the counts and for the scatter) and writes the items (8); pv reads the items and writes pv (12);
           the tree reads pv (4.1) -- 40 bytes per row with one pass (up to 255 documents), 64 with two -- as the rate they were moved at
  count    tc_esa_doc_count_dev at limit 0, 1, 2 against tc_esa_find_dev (first_row and occ, no first_pos) on the same substrings of
           --find-len bytes.  limit 1 is find plus one search over the tree of pv: its ratio is what that search costs.  limit 0 takes
           one search per document found: the mean df is printed beside it, and where it is above 16 the batch is cut so that a call
           lists about 16 * --queries documents (the batch size is printed)
  list     tc_esa_doc_list_dev (sizes, scan, fill) on the same substrings, at a capacity found by a sizes-only call
  kmers    tc_esa_kmer_docs_dev(21), the full list and sizes only, against tc_kmers_esa_dev(21) on the same handle, and
           tc_esa_kmer_doc_spectrum_dev(21) against tc_kmer_spectrum_esa_dev(21, 256 bins)"""
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
    ap.add_argument("--queries", type=int, default=10 ** 7)
    ap.add_argument("--find-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--find-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import textcomp
    ctx = textcomp.Context(0)
    lib, h = ctx.lib, ctx.handle
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(h))
    n, nq, L = 1 << a.log2, a.queries, a.find_len

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
        return statistics.median(ms), min(ms), max(ms)

    def p(t):
        return C.c_void_p(t.data_ptr())

    def line(text):
        print("%-13s | %2d | %s" % (name, a.log2, text), flush=True)

    torch.manual_seed(0xD0C5)
    for kind in a.kinds:
        name = NAMES.get(kind, str(kind))
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        pt = p(d_text)
        assert lib.tc_generate_dev(h, kind, 0xC2, n, pt) == 0
        torch.cuda.synchronize()
        qs, ql = torch.zeros(nq, dtype=torch.int32, device="cuda"), torch.full((nq,), L, dtype=torch.int32, device="cuda")
        out = [torch.empty(nq, dtype=torch.int32, device="cuda") for _ in range(2)]
        fresh = lambda: qs.random_(0, n - L)

        def build_plain():
            hh = C.c_void_p()
            ctx._check(lib.tc_esa_build_dev(h, pt, n, C.byref(hh)))
            lib.tc_esa_free(hh)
        plain_ms, plain_lo, plain_hi = timed(build_plain)
        if a.find_only:
            H = ctx.esa_build_dev(d_text)
            ms, lo, hi = timed(lambda: ctx._check(lib.tc_esa_find_dev(h, H._h, p(qs), p(ql), nq, p(out[0]), p(out[1]), None)), prep=fresh)
            line("tc_esa_build_dev %9.3f ms (%.3f .. %.3f) | find len %d, no first_pos %9.3f ms (%.3f .. %.3f) = %8.1f M queries/s"
                 % (plain_ms, plain_lo, plain_hi, L, ms, lo, hi, nq / ms / 1e3))
            H.close()
            continue
        for ndocs in a.ndocs:
            ds = (np.arange(ndocs + 1, dtype=np.uint64) * n // ndocs).astype(np.uint32)
            tag = "%5d docs" % ndocs

            def build_docs():
                hh = C.c_void_p()
                ctx._check(lib.tc_esa_build_docs_dev(h, pt, n, ds.ctypes.data_as(C.c_void_p), ndocs, C.byref(hh)))
                lib.tc_esa_free(hh)
            docs_ms, _, _ = timed(build_docs)
            part = docs_ms - plain_ms
            model = 40 if ndocs <= 255 else 64
            line("%s | build_docs %9.3f ms | build %9.3f ms (%.3f .. %.3f) | the document part %8.3f ms = %5.1f%% of build | model %d bytes/row = %6.1f GB/s"
                 % (tag, docs_ms, plain_ms, plain_lo, plain_hi, part, 100.0 * part / plain_ms, model, model * (n + 1) / max(part, 1e-3) / 1e6))
            H = ctx.esa_build_docs_dev(d_text, ds)
            line("%s | handle: %d bytes = %.3f per text byte (plain parts %d, da + doc_start %d, pv + tree %d)"
                 % (tag, H.device_bytes(0), H.device_bytes(0) / n, sum(H.device_bytes(k) for k in range(1, 6)), H.device_bytes(6), H.device_bytes(7)))
            eh = H._h
            find_ms, flo, fhi = timed(lambda: ctx._check(lib.tc_esa_find_dev(h, eh, p(qs), p(ql), nq, p(out[0]), p(out[1]), None)), prep=fresh)
            line("%s | find len %d, no first_pos        | %9.3f ms (%.3f .. %.3f) | %8.1f M queries/s" % (tag, L, find_ms, flo, fhi, nq / find_ms / 1e3))
            # the mean df of a small batch decides the batch of the measurements that take one search per document
            probe = min(nq, 10 ** 4)
            fresh()
            torch.cuda.synchronize()
            ctx._check(lib.tc_esa_doc_count_dev(h, eh, p(qs), p(ql), probe, 0, p(out[0]), None))
            mean_df = out[0][:probe].double().mean().item()
            nq0 = nq if mean_df <= 16 else max(probe, int(nq * 16 / mean_df))
            for limit in (1, 2, 0):
                cnt = nq0 if limit == 0 else nq
                ms, lo, hi = timed(lambda: ctx._check(lib.tc_esa_doc_count_dev(h, eh, p(qs), p(ql), cnt, limit, p(out[0]), p(out[1]))), prep=fresh)
                df = out[0][:cnt].double().mean().item()
                base = find_ms * cnt / nq
                line("%s | doc_count limit %d, %8d queries | %9.3f ms (%.3f .. %.3f) | %8.1f M queries/s | x %5.2f of find | mean df %.2f, %8.1f M documents/s"
                     % (tag, limit, cnt, ms, lo, hi, cnt / ms / 1e3, ms / base, df, cnt * df / ms / 1e3))
            # the list: the capacity from a sizes-only call on one batch, with room for the next batches
            offs = torch.empty(nq0 + 1, dtype=torch.int64, device="cuda")
            total = C.c_uint64(0)
            fresh()
            torch.cuda.synchronize()
            rc = lib.tc_esa_doc_list_dev(h, eh, p(qs), p(ql), nq0, 0, p(offs), None, None, C.byref(total))
            assert rc in (0, -2), rc
            cap = int(total.value * 1.5) + 1024
            d_docs, d_hits = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
            got = C.c_uint64(0)
            short = []

            def list_call():
                got.value = cap
                rc = lib.tc_esa_doc_list_dev(h, eh, p(qs), p(ql), nq0, 0, p(offs), p(d_docs), p(d_hits), C.byref(got))
                if rc == -2:
                    short.append(got.value)     # (a batch with half as many documents again as the probe's: its call stopped after the sizes)
                else:
                    ctx._check(rc)
            ms, lo, hi = timed(list_call, prep=fresh)
            if short:
                line("%s | doc_list: not measured, %d of the batches needed more than the %d slots of 1.5 times the probe's total" % (tag, len(short), cap))
            else:
                line("%s | doc_list with hit_pos, %8d queries | %9.3f ms (%.3f .. %.3f) | %8.1f M queries/s | x %5.2f of find | %d documents listed, %8.1f M documents/s"
                     % (tag, nq0, ms, lo, hi, nq0 / ms / 1e3, ms / (find_ms * nq0 / nq), got.value, got.value / ms / 1e3))
            del offs, d_docs, d_hits
            # ---- the k-mers
            k = 21
            kcap = H.kmers(k)[0].numel()
            km_ms, _, _ = timed(lambda: H.kmers(k, cap=kcap))
            kd_ms, _, _ = timed(lambda: H.kmer_docs_dev(k, cap=kcap))
            ks_ms, _, _ = timed(lambda: H.kmer_doc_count(k))
            line("%s | kmers k = %d, %d of them | tc_kmers_esa_dev %8.3f ms | kmer_docs_dev %8.3f ms = x %5.2f | sizes only %8.3f ms"
                 % (tag, k, kcap, km_ms, kd_ms, kd_ms / km_ms, ks_ms))
            sp_ms, _, _ = timed(lambda: H.kmer_spectrum(k, 256))
            ds_ms, _, _ = timed(lambda: H.kmer_doc_spectrum_dev(k))
            hist, distinct = H.kmer_doc_spectrum(k)
            core = int(hist[ndocs])
            line("%s | spectrum k = %d | tc_kmer_spectrum_esa_dev %8.3f ms | kmer_doc_spectrum_dev %8.3f ms = x %5.2f | %d distinct, %d in one document, %d in all"
                 % (tag, k, sp_ms, ds_ms, ds_ms / sp_ms, distinct, int(hist[1]), core))
            H.close()
        del d_text, qs, ql, out


if __name__ == "__main__":
    main()
