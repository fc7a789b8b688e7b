// tc_esa_docs_host.hpp -- host side of the document collections on the kept enhanced suffix array (tc_esa_docs.hpp has the
// kernels and the method): the document part of the handle and its build, and the bodies of tc_esa_build_docs, tc_esa_doc_count,
// tc_esa_doc_list, tc_esa_kmer_docs, tc_esa_kmer_doc_spectrum and their _dev forms.  Included by textcomp.hip after
// tc_esa_host.hpp, whose handle, build and query batch it uses -- the document part is built behind the unchanged build of
// tc_esa_build -- and after tc_kmer_host.hpp, whose scratch and carries the k-mer passes use.
#pragma once
#include "tc_esa_docs.hpp"

static_assert(TC_ESA_NO_DOC == ESD_NO_DOC && TC_ESA_MAX_DOCS == ESD_MAX_DOCS, "include/textcomp.h and tc_esa_docs.hpp state one value each");

// Scratch of the build in the calling context's workspace: the items of the sort, 8 bytes per row and buffer (one buffer per
// pass), and the tiles' digit counts and their scan, 2 * 8 * 256 bytes per tile of ESD_TILE rows.
struct EsdWork {
    u32 ntiles = 0, passes = 0;
    u64 *items[2] = {nullptr, nullptr};
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    void carve(Arena &A, u64 N, u32 ndocs) {
        ntiles = tc_cdiv(N, ESD_TILE);
        passes = ndocs <= 255 ? 1 : 2;          // keys 0 .. ndocs
        for (u32 p = 0; p < passes; p++) items[p] = A.get<u64>(N);
        cnt = A.get<u64>((size_t)256 * ntiles);
        offs = A.get<u64>((size_t)256 * ntiles);
        tsum = A.get<u64>(tc_cdiv((u64)256 * ntiles, SCAN_TILE) + 2);
    }
};

// da, pv and the min tree of pv of a handle whose blocks are allocated and whose doc_start is uploaded
static void esd_build_arrays(tc_ctx *ctx, tc_esa *e) {
    hipStream_t s = ctx->stream;
    const u64 N = e->N;
    EsdWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { W.carve(A, N, e->ndocs); });
    if (e->ndocs + 1 <= ESD_LDS_DOCS)
        esd_da_kernel<true><<<tc_cdiv(N, ESD_NT), ESD_NT, (e->ndocs + 1) * sizeof(u32), s>>>(e->d_sa, N, e->d_doc_start, e->ndocs, e->d_da);
    else
        esd_da_kernel<false><<<tc_cdiv(N, ESD_NT), ESD_NT, 0, s>>>(e->d_sa, N, e->d_doc_start, e->ndocs, e->d_da);
    TC_LAUNCH_CHECK(ctx);
    for (u32 p = 0; p < W.passes; p++) {
        const u32 shift = 8 * p;
        if (p == 0) esd_sort_count_kernel<true><<<W.ntiles, ESD_NT, 0, s>>>(e->d_da, nullptr, N, shift, W.cnt);
        else esd_sort_count_kernel<false><<<W.ntiles, ESD_NT, 0, s>>>(nullptr, W.items[p - 1], N, shift, W.cnt);
        TC_LAUNCH_CHECK(ctx);
        tc_scan64(ctx, W.cnt, (u64)256 * W.ntiles, W.tsum, W.offs);
        if (p == 0) esd_sort_scatter_kernel<true><<<W.ntiles, ESD_NT, 0, s>>>(e->d_da, nullptr, N, shift, W.offs, W.items[p]);
        else esd_sort_scatter_kernel<false><<<W.ntiles, ESD_NT, 0, s>>>(nullptr, W.items[p - 1], N, shift, W.offs, W.items[p]);
        TC_LAUNCH_CHECK(ctx);
    }
    esd_pv_kernel<<<tc_cdiv(N, ESD_NT), ESD_NT, 0, s>>>(W.items[W.passes - 1], N, e->d_pv);
    TC_LAUNCH_CHECK(ctx);
    e->tree.build(ctx, e->d_pv, e->d_pv_min);
}

// tc_esa_build_docs, tc_esa_build_docs_dev
static void esa_build_docs_entry(tc_ctx *ctx, const u8 *text, u64 n, const u32 *doc_start, u32 ndocs, tc_esa **out, bool dev) {
    if (out) *out = nullptr;
    if (!out || n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (ndocs < 1 || ndocs > TC_ESA_MAX_DOCS) TC_FAIL(ctx, TC_ERR_ARG, "ndocs is 1 .. %u", (unsigned)TC_ESA_MAX_DOCS);
    if (!doc_start) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (doc_start[0] != 0 || doc_start[ndocs] != n) TC_FAIL(ctx, TC_ERR_ARG, "doc_start[0] is 0 and doc_start[ndocs] is n");
    for (u32 d = 0; d < ndocs; d++)
        if (doc_start[d] > doc_start[d + 1]) TC_FAIL(ctx, TC_ERR_ARG, "doc_start decreases at document %u", (unsigned)d);
    tc_esa *e = nullptr;
    esa_build_entry(ctx, text, n, &e, dev);
    try {
        e->ndocs = ndocs;
        TC_HIP(ctx, hipMalloc((void **)&e->d_doc_start, esa_doc_start_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_da, esa_rows_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_pv, esa_rows_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_pv_min, esa_tree_bytes(e)));
        tc_h2d(ctx, e->d_doc_start, doc_start, ((size_t)ndocs + 1) * sizeof(u32));
        esd_build_arrays(ctx, e);
        tc_sync_check(ctx);
    } catch (...) {
        esa_release(e);
        throw;
    }
    *out = e;
}

// what every document query checks first
static void esd_check_handle(tc_ctx *ctx, const tc_esa *e) {
    esa_check_handle(ctx, e);
    if (!e->ndocs) TC_FAIL(ctx, TC_ERR_ARG, "the handle has no documents (build it with tc_esa_build_docs)");
}

template <bool FILL>
static void esd_launch(tc_ctx *ctx, const tc_esa *e, const u32 *d_start, const u32 *d_len, u64 nq, u32 limit, u32 *d_df, u32 *d_occ,
                       u64 *d_cnt, const u64 *d_offs, u32 *d_docs, u32 *d_hit, u32 *d_bad) {
    esd_doc_kernel<FILL><<<tc_cdiv(nq, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>((u32)e->n, e->d_sa, e->d_isa, e->d_lcp, e->d_lcp_min, e->d_da, e->d_pv,
                                                                             e->d_pv_min, e->tree.lf, e->ndocs, d_start, d_len, nq, limit, d_df, d_occ,
                                                                             d_cnt, d_offs, d_docs, d_hit, d_bad);
}

// tc_esa_doc_count, tc_esa_doc_count_dev
static void esa_doc_count_entry(tc_ctx *ctx, const tc_esa *e, const u32 *start, const u32 *len, u64 nq, u32 limit, u32 *df, u32 *occ, bool dev) {
    esd_check_handle(ctx, e);
    if (nq == 0) return;
    if (!start || !len || !df) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const void *in[2] = {start, len};
    void *out[2] = {df, occ};
    const u32 size[2] = {4, 4};
    esa_run_batch(ctx, in, 2, out, size, 2, nq, dev, [&](const EsaBatch &B) {
        esd_launch<false>(ctx, e, B.in[0], B.in[1], nq, limit, static_cast<u32 *>(B.out[0]), static_cast<u32 *>(B.out[1]), nullptr, nullptr, nullptr,
                          nullptr, B.d_bad);
    });
}

// tc_esa_doc_list, tc_esa_doc_list_dev: the sizes pass, the scan of the sizes (list_offs[0 .. nq], the last entry the total), the
// host reads the total and the flag, the fill pass -- the capacity protocol of tc_fm_locate
static void esa_doc_list_entry(tc_ctx *ctx, const tc_esa *e, const u32 *start, const u32 *len, u64 nq, u32 limit, u64 *list_offs, u32 *docs,
                               u32 *hit_pos, u64 *ntotal, bool dev) {
    esd_check_handle(ctx, e);
    if (!ntotal) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *ntotal;
    *ntotal = 0;
    if (nq == 0) return;
    if (nq > 0xffffffffull) TC_FAIL(ctx, TC_ERR_ARG, "more than 2^32 - 1 queries in one call");
    if (!start || !len || !list_offs || (!docs && cap)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u32 *d_start = start, *d_len = len;
    u32 *d_bad = nullptr, *d_docs = docs, *d_hit = hit_pos;
    u64 *d_cnt = nullptr, *d_tsum = nullptr, *d_offs = list_offs;
    // The host form stages its lists in the workspace, and only as many slots as the batch lists: the staging is carved behind
    // everything else, in a second plan, once the sizes pass has told the total (out_slots = 0: the first plan).
    auto plan = [&](u64 out_slots) {
        tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
            d_bad = A.get<u32>(1);
            d_cnt = A.get<u64>(nq);
            d_tsum = A.get<u64>(tc_cdiv(nq, SCAN_TILE) + 2);
            if (!dev) {
                d_start = A.get<u32>(nq);
                d_len = A.get<u32>(nq);
                d_offs = A.get<u64>(nq + 1);
                if (out_slots) {
                    d_docs = A.get<u32>(out_slots);
                    d_hit = hit_pos ? A.get<u32>(out_slots) : nullptr;
                }
            }
        });
    };
    hipStream_t s = ctx->stream;
    auto sizes = [&]() -> u64 {     // upload, the count instance, the scan; the host waits for the flag and the total
        tc_memset_async(ctx, d_bad, 0, sizeof(u32));
        if (!dev) {
            tc_h2d(ctx, const_cast<u32 *>(d_start), start, nq * sizeof(u32));
            tc_h2d(ctx, const_cast<u32 *>(d_len), len, nq * sizeof(u32));
        }
        esd_launch<false>(ctx, e, d_start, d_len, nq, limit, nullptr, nullptr, d_cnt, nullptr, nullptr, nullptr, d_bad);
        TC_LAUNCH_CHECK(ctx);
        const u64 *d_total = tc_scan64(ctx, d_cnt, nq, d_tsum, d_offs);
        TC_HIP(ctx, hipMemcpyAsync(d_offs + nq, d_total, sizeof(u64), hipMemcpyDeviceToDevice, s));
        tc_d2h(ctx, &ctx->h_scalars[9], d_total, sizeof(u64));
        tc_d2h(ctx, &ctx->h_scalars[8], d_bad, sizeof(u32));
        tc_sync_check(ctx);
        if ((u32)ctx->h_scalars[8]) TC_FAIL(ctx, TC_ERR_ARG, "a query leaves the text");
        return ctx->h_scalars[9];
    };
    plan(0);
    const u64 need = sizes();
    *ntotal = need;
    if (need > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu document slots, have %llu", (unsigned long long)need, (unsigned long long)cap);
    if (!dev && need) {
        const char *ws = ctx->ws;
        const size_t ws_cap = ctx->ws_cap;
        plan(need);                 // the same carves and the staging behind them
        if (ctx->ws != ws || ctx->ws_cap != ws_cap) sizes();    // the workspace had to grow and may have moved: the first pass again
    }
    if (need) {
        esd_launch<true>(ctx, e, d_start, d_len, nq, limit, nullptr, nullptr, nullptr, d_offs, d_docs, d_hit, d_bad);
        TC_LAUNCH_CHECK(ctx);
    }
    if (!dev) {
        tc_d2h(ctx, list_offs, d_offs, (nq + 1) * sizeof(u64));
        if (need) tc_d2h(ctx, docs, d_docs, need * sizeof(u32));
        if (need && hit_pos) tc_d2h(ctx, hit_pos, d_hit, need * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// ---- the document frequency of the k-mers: tc_esa_kmer_docs, tc_esa_kmer_doc_spectrum and their _dev forms.  Scratch behind
// the handle, in the calling context's workspace: what the k-mer list needs (KmWork of tc_kmer_host.hpp) and 20 bytes per tile
// more -- the tiles' flag totals, their scan and the flags before each tile's last boundary.  Nothing per row.
struct KmdWork {
    KmWork K;
    u64 *fsum = nullptr, *fbase = nullptr, *ftsum = nullptr;
    u32 *inlast = nullptr;
    void carve(Arena &A, u64 N, bool list) {
        K.carve(A, N, list, 0);
        fsum = A.get<u64>(K.ntiles);
        fbase = A.get<u64>(K.ntiles);
        ftsum = A.get<u64>(tc_cdiv(K.ntiles, SCAN_TILE) + 2);
        inlast = A.get<u32>(K.ntiles);
    }
};

static u32 kmd_aligned(const tc_esa *e) { return km_aligned(e->d_lcp) | km_aligned(e->d_pv) << 1; }

// the carries of the boundaries, the tiles' flag totals and their scan: what every pass over the groups starts from
static void kmd_prefixes(tc_ctx *ctx, const KmdWork &W, const tc_esa *e, u32 k) {
    km_carries(ctx, W.K, e->d_lcp, e->N, k);
    kmd_flag_kernel<<<W.K.ntiles, KM_NT, 0, ctx->stream>>>(e->d_lcp, e->d_pv, e->N, k, kmd_aligned(e), W.K.carry, W.fsum, W.inlast);
    TC_LAUNCH_CHECK(ctx);
    tc_scan64(ctx, W.fsum, W.K.ntiles, W.ftsum, W.fbase);
}

// tc_esa_kmer_docs, tc_esa_kmer_docs_dev: count, scan, the host reads the total, fill -- the capacity protocol of tc_kmers_esa_dev
static void esa_kmer_docs_entry(tc_ctx *ctx, const tc_esa *e, u32 k, u32 min_df, u32 max_df, u32 *kpos, u32 *kocc, u32 *kdf, u32 *krow, u64 *nk,
                                bool dev) {
    esd_check_handle(ctx, e);
    if (!nk) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nk;
    *nk = 0;
    if (k == 0 || (max_df != 0 && max_df < min_df)) TC_FAIL(ctx, TC_ERR_ARG, "k is at least 1, max_df is 0 or at least min_df");
    const bool none = !kpos && !kocc && !kdf && !krow, sizes_only = none && cap == 0;
    if (none && !sizes_only) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = e->N, slots = cap < e->n ? cap : e->n;       // (a text of n bytes has at most n k-mers)
    u32 *out[4] = {kpos, kocc, kdf, krow}, *d_out[4] = {kpos, kocc, kdf, krow};
    KmdWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        W.carve(A, N, true);
        if (!dev)
            for (int i = 0; i < 4; i++) d_out[i] = out[i] ? A.get<u32>(slots + 1) : nullptr;
    });
    hipStream_t s = ctx->stream;
    const u32 al = kmd_aligned(e);
    kmd_prefixes(ctx, W, e, k);
    kmd_pass_kernel<KM_COUNT><<<W.K.ntiles, KM_NT, 0, s>>>(e->d_sa, e->d_lcp, e->d_pv, N, k, min_df, max_df, al, W.K.carry, W.fbase, W.inlast, W.K.cnt,
                                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, W.K.cnt, W.K.ntiles, W.K.tsum, W.K.offs, cap, sizes_only, nk, "k-mer");
    if (!sizes_only && need) {
        kmd_pass_kernel<KM_FILL><<<W.K.ntiles, KM_NT, 0, s>>>(e->d_sa, e->d_lcp, e->d_pv, N, k, min_df, max_df, al, W.K.carry, W.fbase, W.inlast, nullptr,
                                                             W.K.offs, d_out[0], d_out[1], d_out[2], d_out[3], nullptr, 0, nullptr);
        TC_LAUNCH_CHECK(ctx);
        if (!dev)
            for (int i = 0; i < 4; i++)
                if (out[i]) tc_d2h(ctx, out[i], d_out[i], need * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// tc_esa_kmer_doc_spectrum, tc_esa_kmer_doc_spectrum_dev: hist[d] = the distinct k-mers that occur in exactly d documents
static void esa_kmer_doc_spectrum_entry(tc_ctx *ctx, const tc_esa *e, u32 k, u64 *hist, u64 *distinct, bool dev) {
    esd_check_handle(ctx, e);
    if (!hist || !distinct) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (k == 0) TC_FAIL(ctx, TC_ERR_ARG, "k is at least 1");
    *distinct = 0;
    const u32 bins = e->ndocs + 1;
    u64 *d_hist = hist;
    KmdWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        W.carve(A, e->N, false);
        if (!dev) d_hist = A.get<u64>(bins);
    });
    tc_memset_async(ctx, d_hist, 0, (size_t)bins * sizeof(u64));
    tc_memset_async(ctx, W.K.word, 0, sizeof(u64));
    kmd_prefixes(ctx, W, e, k);
    kmd_pass_kernel<KM_HIST><<<W.K.ntiles, KM_NT, 0, ctx->stream>>>(e->d_sa, e->d_lcp, e->d_pv, e->N, k, 1u, 0u, kmd_aligned(e), W.K.carry, W.fbase,
                                                                   W.inlast, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_hist, bins, W.K.word);
    TC_LAUNCH_CHECK(ctx);
    if (!dev) tc_d2h(ctx, hist, d_hist, (size_t)bins * sizeof(u64));
    tc_d2h(ctx, &ctx->h_scalars[9], W.K.word, sizeof(u64));
    tc_sync_check(ctx);
    *distinct = ctx->h_scalars[9];
}
