// tc_esa_xdoc_host.hpp -- host side of the cross-document matches on the kept enhanced suffix array (tc_esa_xdoc.hpp has the
// kernels and the method): the scratch, the launch sequences and the bodies of tc_esa_doc_match, tc_esa_doc_shared and their
// _dev forms.  Included by textcomp.hip after tc_esa_docs_host.hpp, whose handle check it uses, and after tc_cov_host.hpp and
// tc_sus_host.hpp, whose kernels the per-document sums and the run heads launch unchanged.  The handle is only read: all
// scratch is the calling context's workspace.
#pragma once
#include "tc_esa_xdoc.hpp"

static_assert(TC_DOC_OTHER == ESX_OTHER && TC_DOC_EARLIER == ESX_EARLIER && TC_ESA_NO_POS == ESX_NO_POS,
              "include/textcomp.h and tc_esa_xdoc.hpp state one value each");

// Scratch of the match: OTHER holds up and dn, 8 bytes per row, and 8 bytes per tile of ESX_TILE rows; EARLIER the min tree
// of da, 4 / (f - 1) bytes per row, of the handle's shape.
struct EsxWork {
    u32 ntiles = 0;
    u32 *up = nullptr, *dn = nullptr, *tlast = nullptr, *tfirst = nullptr, *da_min = nullptr;
    void carve(Arena &A, const tc_esa *e, int kind) {
        if (kind == ESX_OTHER) {
            ntiles = tc_cdiv(e->N, ESX_TILE);
            up = A.get<u32>(e->N);
            dn = A.get<u32>(e->N);
            tlast = A.get<u32>(ntiles);
            tfirst = A.get<u32>(ntiles);
        } else {
            da_min = A.get<u32>(e->tree.words);
        }
    }
};

// the neighbours' arrays or tree, then the match, n >= 1; each output may be null
static void esx_match(tc_ctx *ctx, const tc_esa *e, const EsxWork &W, int kind, u32 clamp, u32 *d_xl, u32 *d_src, u32 *d_xdoc) {
    hipStream_t s = ctx->stream;
    const u32 N = (u32)e->N, grid = tc_cdiv(e->n, FM_MS_NT);
    if (kind == ESX_OTHER) {
        esx_reduce_kernel<<<W.ntiles, ESX_NT, 0, s>>>(e->d_da, N, W.tlast, W.tfirst);
        TC_LAUNCH_CHECK(ctx);
        sus_spine_kernel<<<1, 1024, 0, s>>>(W.tlast, W.tfirst, W.ntiles, N);
        TC_LAUNCH_CHECK(ctx);
        esx_heads_kernel<<<W.ntiles, ESX_NT, 0, s>>>(e->d_da, N, W.tlast, W.tfirst, W.up, W.dn);
        TC_LAUNCH_CHECK(ctx);
        esx_match_kernel<ESX_OTHER><<<grid, FM_MS_NT, 0, s>>>((u32)e->n, e->d_sa, e->d_lcp, e->d_lcp_min, e->d_da, nullptr, W.up, W.dn, e->d_doc_start,
                                                               e->ndocs, e->tree.lf, clamp, d_xl, d_src, d_xdoc);
    } else {
        e->tree.build(ctx, e->d_da, W.da_min);
        esx_match_kernel<ESX_EARLIER><<<grid, FM_MS_NT, 0, s>>>((u32)e->n, e->d_sa, e->d_lcp, e->d_lcp_min, e->d_da, W.da_min, nullptr, nullptr,
                                                                 e->d_doc_start, e->ndocs, e->tree.lf, clamp, d_xl, d_src, d_xdoc);
    }
    TC_LAUNCH_CHECK(ctx);
}

static void esx_check(tc_ctx *ctx, const tc_esa *e, int kind) {
    esd_check_handle(ctx, e);
    if (kind != TC_DOC_OTHER && kind != TC_DOC_EARLIER) TC_FAIL(ctx, TC_ERR_ARG, "kind is TC_DOC_OTHER or TC_DOC_EARLIER");
}

// tc_esa_doc_match, tc_esa_doc_match_dev
static void esa_doc_match_entry(tc_ctx *ctx, const tc_esa *e, int kind, int clamp, u32 *xl, u32 *src, u32 *xdoc, bool dev) {
    esx_check(ctx, e, kind);
    const u64 n = e->n;
    if (n == 0) return;
    if (!xl && !src && !xdoc) TC_FAIL(ctx, TC_ERR_ARG, "xl, src and xdoc are all null");
    u32 *out[3] = {xl, src, xdoc}, *d_out[3] = {xl, src, xdoc};
    EsxWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        W.carve(A, e, kind);
        if (!dev)
            for (int k = 0; k < 3; k++) d_out[k] = out[k] ? A.get<u32>(n) : nullptr;
    });
    esx_match(ctx, e, W, kind, clamp ? 1u : 0u, d_out[0], d_out[1], d_out[2]);
    if (!dev)
        for (int k = 0; k < 3; k++)
            if (out[k]) tc_d2h(ctx, out[k], d_out[k], n * sizeof(u32));
    tc_sync_check(ctx);
}

// Scratch of the per-document answers behind the match's: the clamped lengths, 4 bytes per text byte; for shared the cover, 1
// byte per text byte, the cover core's tile maxima, the tile sums and their scan, and the ndocs + 1 prefixes; for longest 8 bytes
// per tile of ESX_TILE positions.
struct EsxDocWork {
    EsxWork M;
    u32 ctiles = 0, stiles = 0, ptiles = 0;
    u32 *len = nullptr, *tmax = nullptr;
    u8 *cov = nullptr;
    u64 *tsum = nullptr, *tbase = nullptr, *ttsum = nullptr, *pre = nullptr, *pair = nullptr;
    void carve(Arena &A, const tc_esa *e, int kind, bool shared, bool longest) {
        M.carve(A, e, kind);
        len = A.get<u32>(e->n);
        if (shared) {
            ctiles = tc_cdiv(e->n, COV_TILE);
            stiles = tc_cdiv(e->n, ESX_STILE) + 1;      // (one tile behind the last: a boundary at n may stand there)
            cov = A.get<u8>(e->n + 16);
            tmax = A.get<u32>(ctiles);
            tsum = A.get<u64>(stiles);
            tbase = A.get<u64>(stiles);
            ttsum = A.get<u64>(tc_cdiv(stiles, SCAN_TILE) + 2);
            pre = A.get<u64>((size_t)e->ndocs + 1);
        }
        if (longest) {
            ptiles = tc_cdiv(e->n, ESX_TILE);
            pair = A.get<u64>(ptiles);
        }
    }
};

// tc_esa_doc_shared, tc_esa_doc_shared_dev
static void esa_doc_shared_entry(tc_ctx *ctx, const tc_esa *e, int kind, u32 min_len, u64 *shared, u32 *longest, bool dev) {
    esx_check(ctx, e, kind);
    if (min_len == 0) TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 1");
    if (!shared && !longest) TC_FAIL(ctx, TC_ERR_ARG, "shared and longest are both null");
    const u64 n = e->n;
    const u32 ndocs = e->ndocs, n32 = (u32)n;
    if (n == 0) {       // every document is empty
        if (!dev) {
            if (shared) memset(shared, 0, (size_t)ndocs * sizeof(u64));
            if (longest) memset(longest, 0, (size_t)ndocs * sizeof(u32));
            return;
        }
        if (shared) tc_memset_async(ctx, shared, 0, (size_t)ndocs * sizeof(u64));
        if (longest) tc_memset_async(ctx, longest, 0, (size_t)ndocs * sizeof(u32));
        tc_sync_check(ctx);
        return;
    }
    u64 *d_shared = shared;
    u32 *d_longest = longest;
    EsxDocWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        W.carve(A, e, kind, shared != nullptr, longest != nullptr);
        if (!dev) {
            d_shared = shared ? A.get<u64>(ndocs) : nullptr;
            d_longest = longest ? A.get<u32>(ndocs) : nullptr;
        }
    });
    hipStream_t s = ctx->stream;
    esx_match(ctx, e, W.M, kind, 1u, W.len, nullptr, nullptr);
    if (shared && min_len > n) {            // no position counts
        tc_memset_async(ctx, d_shared, 0, (size_t)ndocs * sizeof(u64));
    } else if (shared) {
        cov_reduce_kernel<<<W.ctiles, COV_NT, 0, s>>>(W.len, n32, min_len, W.tmax);
        TC_LAUNCH_CHECK(ctx);
        cov_spine_kernel<<<1, 1024, 0, s>>>(W.tmax, W.ctiles);
        TC_LAUNCH_CHECK(ctx);
        cov_mask_kernel<<<W.ctiles, COV_NT, 0, s>>>(W.len, n32, min_len, W.tmax, nullptr, CovMap{}, 0u, W.cov);
        TC_LAUNCH_CHECK(ctx);
        esx_tile_sum_kernel<<<W.stiles, ESX_NT, 0, s>>>(W.cov, n, W.tsum);
        TC_LAUNCH_CHECK(ctx);
        tc_scan64(ctx, W.tsum, W.stiles, W.ttsum, W.tbase);
        esx_doc_prefix_kernel<<<ndocs + 1, ESX_NT, 0, s>>>(W.cov, n, e->d_doc_start, W.tbase, W.pre);
        TC_LAUNCH_CHECK(ctx);
        esx_doc_diff_kernel<<<tc_cdiv(ndocs, ESX_NT), ESX_NT, 0, s>>>(W.pre, ndocs, d_shared);
        TC_LAUNCH_CHECK(ctx);
    }
    if (longest) {
        tc_memset_async(ctx, d_longest, 0, (size_t)ndocs * sizeof(u32));    // (a document that ends at position 0 is in no tile)
        esx_seg_kernel<0><<<W.ptiles, ESX_NT, 0, s>>>(W.len, n32, e->d_doc_start, ndocs, W.pair, nullptr);
        TC_LAUNCH_CHECK(ctx);
        esx_seg_spine_kernel<<<1, 1024, 0, s>>>(W.pair, W.ptiles);
        TC_LAUNCH_CHECK(ctx);
        esx_seg_kernel<1><<<W.ptiles, ESX_NT, 0, s>>>(W.len, n32, e->d_doc_start, ndocs, W.pair, d_longest);
        TC_LAUNCH_CHECK(ctx);
    }
    if (!dev) {
        if (shared) tc_d2h(ctx, shared, d_shared, (size_t)ndocs * sizeof(u64));
        if (longest) tc_d2h(ctx, longest, d_longest, (size_t)ndocs * sizeof(u32));
    }
    tc_sync_check(ctx);
}
