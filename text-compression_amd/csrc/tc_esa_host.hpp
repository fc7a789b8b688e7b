// tc_esa_host.hpp -- host side of the kept enhanced suffix array (tc_esa.hpp has the kernels and the method): the handle, its
// build, tc_esa_read, and the bodies of tc_esa_lce / tc_esa_find / tc_esa_compare and their _dev forms.  Included by textcomp.hip
// after tc_esa_plan.hpp; the build is its lower layer (esa_sort: the workspace holds scratch only, the arrays are the handle's
// own), then lcp_device, tr_isa_kernel and the two min trees.
#pragma once
#include "tc_esa.hpp"

static_assert(TC_ESA_MAX_MISMATCH == ESA_MAX_MISMATCH, "esa_lce_kernel takes at most TC_ESA_MAX_MISMATCH turns and one");

// The handle: its own hipMalloc blocks, read-only after the build.  Per text byte: 1 (text) + 4 (sa) + 4 (isa) + 4 (lcp) and
// 4 / (f - 1) for each of the two min trees of fan-out f -- 13.13 at f = 64.  Every block is rounded up to 16 bytes, the text
// has 16 more behind it: the 16-byte loads of the searches stay inside the blocks.
struct tc_esa {
    int device = 0;
    u64 n = 0, N = 0;
    MinTree tree;               // both trees are over the N rows: one shape
    u8 *d_text = nullptr;
    u32 *d_sa = nullptr, *d_isa = nullptr, *d_lcp = nullptr, *d_lcp_min = nullptr, *d_sa_min = nullptr;
    // the document part (tc_esa_docs_host.hpp; ndocs = 0: a plain handle, the four blocks null): doc_start, ndocs + 1 entries,
    // da and pv, N entries each, and the min tree of pv -- 8 + 4 / (f - 1) bytes per text byte more
    u32 ndocs = 0;
    u32 *d_doc_start = nullptr, *d_da = nullptr, *d_pv = nullptr, *d_pv_min = nullptr;
};

static u64 esa_text_bytes(const tc_esa *e) { return (e->n + 16 + 15) & ~(u64)15; }
static u64 esa_rows_bytes(const tc_esa *e) { return (e->N * sizeof(u32) + 15) & ~(u64)15; }
static u64 esa_tree_bytes(const tc_esa *e) { return (u64)e->tree.words * sizeof(u32); }
static u64 esa_doc_start_bytes(const tc_esa *e) { return (((u64)e->ndocs + 1) * sizeof(u32) + 15) & ~(u64)15; }

static void esa_release(tc_esa *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->d_text) (void)hipFree(e->d_text);
    if (e->d_sa) (void)hipFree(e->d_sa);
    if (e->d_isa) (void)hipFree(e->d_isa);
    if (e->d_lcp) (void)hipFree(e->d_lcp);
    if (e->d_lcp_min) (void)hipFree(e->d_lcp_min);
    if (e->d_sa_min) (void)hipFree(e->d_sa_min);
    if (e->d_doc_start) (void)hipFree(e->d_doc_start);
    if (e->d_da) (void)hipFree(e->d_da);
    if (e->d_pv) (void)hipFree(e->d_pv);
    if (e->d_pv_min) (void)hipFree(e->d_pv_min);
    delete e;
}

// tc_esa_device_bytes: 0 all, 1 text, 2 sa, 3 isa, 4 lcp + its min tree, 5 the min tree of sa; on a handle with documents
// 6 da + doc_start, 7 pv + its min tree (0 on a plain one)
static u64 esa_device_bytes(const tc_esa *e, int part) {
    if (!e) return 0;
    switch (part) {
    case 0: return esa_text_bytes(e) + 3 * esa_rows_bytes(e) + 2 * esa_tree_bytes(e) + esa_device_bytes(e, 6) + esa_device_bytes(e, 7);
    case 6: return e->ndocs ? esa_rows_bytes(e) + esa_doc_start_bytes(e) : 0;
    case 7: return e->ndocs ? esa_rows_bytes(e) + esa_tree_bytes(e) : 0;
    case 1: return esa_text_bytes(e);
    case 2: case 3: return esa_rows_bytes(e);
    case 4: return esa_rows_bytes(e) + esa_tree_bytes(e);
    case 5: return esa_tree_bytes(e);
    default: return 0;
    }
}

// tc_esa_build, tc_esa_build_dev
static void esa_build_entry(tc_ctx *ctx, const u8 *text, u64 n, tc_esa **out, bool dev) {
    if (out) *out = nullptr;
    if (!out || n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n && !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    tc_esa *e = new tc_esa();
    e->device = ctx->device;
    e->n = n;
    e->N = N;
    try {
        hipStream_t s = ctx->stream;
        e->tree.shape(ctx, (u32)N);
        TC_HIP(ctx, hipMalloc((void **)&e->d_text, esa_text_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_sa, esa_rows_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_isa, esa_rows_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_lcp, esa_rows_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_lcp_min, esa_tree_bytes(e)));
        TC_HIP(ctx, hipMalloc((void **)&e->d_sa_min, esa_tree_bytes(e)));
        tc_memset_async(ctx, e->d_text + n, 0, esa_text_bytes(e) - n);
        if (n) {
            if (dev) TC_HIP(ctx, hipMemcpyAsync(e->d_text, text, n, hipMemcpyDeviceToDevice, s));
            else tc_h2d(ctx, e->d_text, text, n);
            ctx->stats = tc_stats{};
            ctx->stats.n = n; ctx->stats.N = N;
            LcpScratch lcp_ws;
            tc_ws_plan(ctx, 0, [&](Arena &A, bool dry) { esa_sort(ctx, A, e->d_text, n, e->d_sa, lcp_ws, dry); });
            lcp_device(ctx, lcp_ws, e->d_text, n, e->d_sa, e->d_lcp);
        } else {    // the one-row ESA, as tc_suffix_array_dev and tc_lcp_array_dev make it
            tc_memset_async(ctx, e->d_sa, 0, sizeof(u32));
            tc_memset_async(ctx, e->d_lcp, 0, sizeof(u32));
        }
        tr_isa_kernel<<<tc_cdiv(N, TR_NT), TR_NT, 0, s>>>(e->d_sa, (u32)N, e->d_isa, ctx->d_err);
        TC_LAUNCH_CHECK(ctx);
        e->tree.build(ctx, e->d_lcp, e->d_lcp_min);
        e->tree.build(ctx, e->d_sa, e->d_sa_min);
        tc_sync_check(ctx);
    } catch (...) {
        esa_release(e);
        throw;
    }
    *out = e;
}

// what every call on a handle checks first
static void esa_check_handle(tc_ctx *ctx, const tc_esa *e) {
    if (!e) TC_FAIL(ctx, TC_ERR_ARG, "null handle");
    if (e->device != ctx->device) TC_FAIL(ctx, TC_ERR_ARG, "the handle lives on device %d, the context on device %d", e->device, ctx->device);
}

// tc_esa_read: entries [first, first + count) of one array to host or device memory
static void esa_read_entry(tc_ctx *ctx, const tc_esa *e, int what, u64 first, u64 count, void *dst, bool dst_on_device) {
    esa_check_handle(ctx, e);
    if (what < 1 || what > (e->ndocs ? 7 : 4))
        TC_FAIL(ctx, TC_ERR_ARG, "what is 1 (text), 2 (sa), 3 (isa) or 4 (lcp); on a handle with documents also 5 (da), 6 (pv), 7 (doc_start)");
    const u64 have = what == 1 ? e->n : what == 7 ? (u64)e->ndocs + 1 : e->N, size = what == 1 ? 1 : sizeof(u32);
    if (first > have || count > have - first) TC_FAIL(ctx, TC_ERR_ARG, "the range leaves the array (%llu entries)", (unsigned long long)have);
    if (count == 0) return;
    if (!dst) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u32 *rows[8] = {nullptr, nullptr, e->d_sa, e->d_isa, e->d_lcp, e->d_da, e->d_pv, e->d_doc_start};
    const u8 *src = what == 1 ? e->d_text : reinterpret_cast<const u8 *>(rows[what]);
    TC_HIP(ctx, hipMemcpyAsync(dst, src + first * size, count * size, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                               ctx->stream));
    tc_sync_check(ctx);
}

// One batch of queries: up to four input arrays and three output arrays of nq entries (4 bytes each but the int8 order), the
// caller's (dev) or the workspace's, and the word a refused query sets.
struct EsaBatch {
    const u32 *in[4] = {};
    void *out[3] = {};
    u32 *d_bad = nullptr;
};

// carve, upload, launch(B), download, and the flag: a query out of range is TC_ERR_ARG in both forms
template <class F>
static void esa_run_batch(tc_ctx *ctx, const void *const *in, int nin, void *const *out, const u32 *out_size, int nout, u64 nq, bool dev,
                          F &&launch) {
    if (nq > 0xffffffffull) TC_FAIL(ctx, TC_ERR_ARG, "more than 2^32 - 1 queries in one call");
    EsaBatch B;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        B.d_bad = A.get<u32>(1);
        for (int k = 0; k < nin; k++) B.in[k] = dev ? static_cast<const u32 *>(in[k]) : A.get<u32>(nq);
        for (int k = 0; k < nout; k++) B.out[k] = !out[k] ? nullptr : dev ? out[k] : static_cast<void *>(A.get<u8>(nq * out_size[k]));
    });
    tc_memset_async(ctx, B.d_bad, 0, sizeof(u32));
    if (!dev)
        for (int k = 0; k < nin; k++) tc_h2d(ctx, const_cast<u32 *>(B.in[k]), in[k], nq * sizeof(u32));
    launch(B);
    TC_LAUNCH_CHECK(ctx);
    if (!dev)
        for (int k = 0; k < nout; k++)
            if (out[k]) tc_d2h(ctx, out[k], B.out[k], nq * out_size[k]);
    tc_d2h(ctx, &ctx->h_scalars[8], B.d_bad, sizeof(u32));
    tc_sync_check(ctx);
    if ((u32)ctx->h_scalars[8]) TC_FAIL(ctx, TC_ERR_ARG, "a query leaves the text");
}

// tc_esa_lce, tc_esa_lce_dev
static void esa_lce_entry(tc_ctx *ctx, const tc_esa *e, const u32 *a, const u32 *b, u64 nq, u32 max_mismatch, u32 *len, u32 *mm, bool dev) {
    esa_check_handle(ctx, e);
    if (max_mismatch > TC_ESA_MAX_MISMATCH) TC_FAIL(ctx, TC_ERR_ARG, "max_mismatch is at most %u", (unsigned)TC_ESA_MAX_MISMATCH);
    if (nq == 0) return;
    if (!a || !b || !len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const void *in[2] = {a, b};
    void *out[2] = {len, mm};
    const u32 size[2] = {4, 4};
    esa_run_batch(ctx, in, 2, out, size, 2, nq, dev, [&](const EsaBatch &B) {
        esa_lce_kernel<<<tc_cdiv(nq, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>(e->d_text, (u32)e->n, e->d_isa, e->d_lcp, e->d_lcp_min, e->tree.lf, B.in[0],
                                                                          B.in[1], nq, max_mismatch, static_cast<u32 *>(B.out[0]),
                                                                          static_cast<u32 *>(B.out[1]), B.d_bad);
    });
}

// tc_esa_find, tc_esa_find_dev
static void esa_find_entry(tc_ctx *ctx, const tc_esa *e, const u32 *start, const u32 *len, u64 nq, u32 *first_row, u32 *occ, u32 *first_pos,
                           bool dev) {
    esa_check_handle(ctx, e);
    if (nq == 0) return;
    if (!start || !len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (!first_row && !occ && !first_pos) TC_FAIL(ctx, TC_ERR_ARG, "first_row, occ and first_pos are all null");
    const void *in[2] = {start, len};
    void *out[3] = {first_row, occ, first_pos};
    const u32 size[3] = {4, 4, 4};
    esa_run_batch(ctx, in, 2, out, size, 3, nq, dev, [&](const EsaBatch &B) {
        esa_find_kernel<<<tc_cdiv(nq, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>((u32)e->n, e->d_sa, e->d_isa, e->d_lcp, e->d_sa_min, e->d_lcp_min,
                                                                           e->tree.lf, B.in[0], B.in[1], nq, static_cast<u32 *>(B.out[0]),
                                                                           static_cast<u32 *>(B.out[1]), static_cast<u32 *>(B.out[2]),
                                                                           B.d_bad);
    });
}

// tc_esa_compare, tc_esa_compare_dev
static void esa_compare_entry(tc_ctx *ctx, const tc_esa *e, const u32 *a_start, const u32 *a_len, const u32 *b_start, const u32 *b_len,
                              u64 nq, signed char *order, u32 *common, bool dev) {
    esa_check_handle(ctx, e);
    if (nq == 0) return;
    if (!a_start || !a_len || !b_start || !b_len || !order) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const void *in[4] = {a_start, a_len, b_start, b_len};
    void *out[2] = {order, common};
    const u32 size[2] = {1, 4};
    esa_run_batch(ctx, in, 4, out, size, 2, nq, dev, [&](const EsaBatch &B) {
        esa_compare_kernel<<<tc_cdiv(nq, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>(e->d_text, (u32)e->n, e->d_isa, e->d_lcp, e->d_lcp_min, e->tree.lf,
                                                                              B.in[0], B.in[1], B.in[2], B.in[3], nq,
                                                                              static_cast<signed char *>(B.out[0]),
                                                                              static_cast<u32 *>(B.out[1]), B.d_bad);
    });
}
