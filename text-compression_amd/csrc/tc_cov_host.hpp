// tc_cov_host.hpp -- host side of the repeat cover (tc_cov.hpp has the kernels and the method): scratch, the launch sequence, and
// the bodies of tc_repeat_spans / tc_repeat_mask / tc_repeat_dedup, their _dev forms and the three tc_cover_*_dev calls over a
// caller's array of lengths.  Included by textcomp.hip after tc_esa_plan.hpp: the ESA is esa_plan's, with nothing kept but sa
// and lcp.
#pragma once
#include "tc_cov.hpp"

// What the cover core holds over an array of n lengths: 4 bytes per tile of COV_TILE positions for the maxima and 32 for the two
// counts and their scans.
struct CovCore {
    u32 ntiles = 0;
    u32 *tmax = nullptr;
    u64 *cnt_s = nullptr, *cnt_c = nullptr, *offs_s = nullptr, *offs_c = nullptr, *tsum_s = nullptr, *tsum_c = nullptr;
    void carve(Arena &A, u64 n) {
        ntiles = tc_cdiv(n, COV_TILE);
        tmax = A.get<u32>(ntiles);
        cnt_s = A.get<u64>(ntiles);
        cnt_c = A.get<u64>(ntiles);
        offs_s = A.get<u64>(ntiles + 1);
        offs_c = A.get<u64>(ntiles + 1);
        tsum_s = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
        tsum_c = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
    }
};

// What one text call holds in the workspace: the text (host form), sa and lcp (4 + 4 bytes per text byte) and what a host form
// returns ahead of the overlay mark; behind it, over the sort's and then the LCP's dead buffers, len (4 bytes per text byte), the
// min tree of lcp (4 / (f - 1); only where a row is searched: q > 2, or LATER), that of sa (the same; LATER only) and the core's
// tiles: 12 bytes per text byte and a little -- the sort's own need behind the first 8 where that is larger.
struct CovWork : Esa {
    MinTree tree;           // both trees are over the N = n + 1 rows
    u32 *len = nullptr, *lcp_min = nullptr, *sa_min = nullptr;
    CovCore core;
    void carve(const tc_ctx *ctx, Arena &A, u64 n, bool search, bool later) {
        len = A.get<u32>(n);
        tree.shape(ctx, (u32)(n + 1));
        if (search) lcp_min = A.get<u32>(tree.words);
        if (later) sa_min = A.get<u32>(tree.words);
        core.carve(A, n);
    }
};

// what a call is after, and where it goes
enum { COV_SPANS = 0, COV_MASK = 1, COV_DEDUP = 2 };
struct CovCall {
    int what = COV_SPANS;
    u32 *span_start = nullptr, *span_len = nullptr;     // COV_SPANS
    const u8 *map = nullptr;                            // COV_MASK: a host array of 256 bytes, or null
    u8 *out = nullptr;                                  // COV_MASK, COV_DEDUP
    u64 *count = nullptr;                               // COV_SPANS: nspans; COV_DEDUP: nout
    u64 *covered = nullptr;
    u64 cap = 0;                                        // (filled by cov_validate)
    bool sizes_only = false;
};

static bool cov_overlap(const void *a, u64 na, const void *b, u64 nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

// the argument errors every entry shares, before a buffer is touched; text: what the mask and the dedup read (may be null)
static void cov_validate(tc_ctx *ctx, CovCall &c, const u8 *text, u64 n, u32 min_len) {
    if (n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (min_len == 0) TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 1");
    if (c.what == COV_SPANS) {
        if (!c.count) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
        c.cap = *c.count;
        c.sizes_only = !c.span_start && !c.span_len && c.cap == 0;
        if (!c.sizes_only && (!c.span_start || !c.span_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    } else if (c.what == COV_MASK) {
        if (n && !c.out) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
        if (c.map && n && !text) TC_FAIL(ctx, TC_ERR_ARG, "a map needs the text");
        if (cov_overlap(c.out, n, text, n)) TC_FAIL(ctx, TC_ERR_ARG, "out overlaps the text");
    } else {
        if (!c.count) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
        c.cap = *c.count;
        c.sizes_only = !c.out && c.cap == 0;
        if (!c.out && c.cap) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
        if (n && !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
        if (cov_overlap(c.out, c.cap < n ? c.cap : n, text, n)) TC_FAIL(ctx, TC_ERR_ARG, "out overlaps the text");
    }
    if (c.count) *c.count = 0;
    if (c.covered) *c.covered = 0;
}

// a text without a cover (n = 0, or min_len > n): no span, the mask is the text (or zeroes), the dedup is the text
static void cov_nothing_covered(tc_ctx *ctx, const CovCall &c, const u8 *text, u64 n, bool dev) {
    if (c.what == COV_SPANS || n == 0) return;
    if (c.what == COV_DEDUP) {
        *c.count = n;
        if (c.sizes_only) return;
        if (n > c.cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu bytes, have %llu", (unsigned long long)n, (unsigned long long)c.cap);
    }
    const bool copy = c.what == COV_DEDUP || c.map;
    if (!dev) {
        if (copy) memcpy(c.out, text, n); else memset(c.out, 0, n);
        return;
    }
    if (copy) TC_HIP(ctx, hipMemcpyAsync(c.out, text, n, hipMemcpyDeviceToDevice, ctx->stream));
    else tc_memset_async(ctx, c.out, 0, n);
    tc_sync_check(ctx);
}

// The cover of d_len[0 .. n) at min_len, n >= 1, and what the call asks of it.  d_text: the text on the device (null where it
// is not read).  d_start / d_slen / d_out: where the device writes -- the caller's arrays (dev) or the workspace's, which are
// then copied to the caller's host arrays.
static void cov_finish(tc_ctx *ctx, const CovCore &C, const u32 *d_len, const u8 *d_text, u64 n, u32 min_len, const CovCall &c,
                       u32 *d_start, u32 *d_slen, u8 *d_out, bool dev) {
    hipStream_t s = ctx->stream;
    const u32 n32 = (u32)n;
    cov_reduce_kernel<<<C.ntiles, COV_NT, 0, s>>>(d_len, n32, min_len, C.tmax);
    TC_LAUNCH_CHECK(ctx);
    cov_spine_kernel<<<1, 1024, 0, s>>>(C.tmax, C.ntiles);
    TC_LAUNCH_CHECK(ctx);
    cov_count_kernel<<<C.ntiles, COV_NT, 0, s>>>(d_len, n32, min_len, C.tmax, C.cnt_s, C.cnt_c);
    TC_LAUNCH_CHECK(ctx);
    const u64 *d_spans = tc_scan64(ctx, C.cnt_s, C.ntiles, C.tsum_s, C.offs_s);
    const u64 *d_cov = tc_scan64(ctx, C.cnt_c, C.ntiles, C.tsum_c, C.offs_c);
    tc_d2h(ctx, &ctx->h_scalars[9], d_spans, sizeof(u64));
    tc_d2h(ctx, &ctx->h_scalars[8], d_cov, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    const u64 nspans = ctx->h_scalars[9], covered = ctx->h_scalars[8] < n ? ctx->h_scalars[8] : n;
    if (c.covered) *c.covered = covered;
    if (c.what == COV_SPANS) {
        *c.count = nspans;
        if (nspans > c.cap && !c.sizes_only) {
            tc_sync_check(ctx);
            TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu span slots, have %llu", (unsigned long long)nspans, (unsigned long long)c.cap);
        }
        if (!c.sizes_only && nspans) {
            cov_fill_kernel<<<C.ntiles, COV_NT, 0, s>>>(d_len, n32, min_len, C.tmax, C.offs_s, nspans, d_start, d_slen);
            TC_LAUNCH_CHECK(ctx);
            cov_len_kernel<<<tc_cdiv(nspans, 256), 256, 0, s>>>(d_start, d_slen, nspans);
            TC_LAUNCH_CHECK(ctx);
            if (!dev) {
                tc_d2h(ctx, c.span_start, d_start, nspans * sizeof(u32));
                tc_d2h(ctx, c.span_len, d_slen, nspans * sizeof(u32));
            }
        }
    } else if (c.what == COV_MASK) {
        CovMap map = {};
        if (c.map) memcpy(map.w, c.map, 256);
        cov_mask_kernel<<<C.ntiles, COV_NT, 0, s>>>(d_len, n32, min_len, C.tmax, d_text, map, c.map ? 1u : 0u, d_out);
        TC_LAUNCH_CHECK(ctx);
        if (!dev) tc_d2h(ctx, c.out, d_out, n);
    } else {
        const u64 need = n - covered;
        *c.count = need;
        if (need > c.cap && !c.sizes_only) {
            tc_sync_check(ctx);
            TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu bytes, have %llu", (unsigned long long)need, (unsigned long long)c.cap);
        }
        if (!c.sizes_only && need) {
            cov_dedup_kernel<<<C.ntiles, COV_NT, 0, s>>>(d_len, n32, min_len, C.tmax, d_text, C.offs_c, need, d_out);
            TC_LAUNCH_CHECK(ctx);
            if (!dev) tc_d2h(ctx, c.out, d_out, need);
        }
    }
    tc_sync_check(ctx);
}

// tc_repeat_spans, tc_repeat_mask, tc_repeat_dedup and their _dev forms
static void repeat_cover_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 min_len, u32 min_occ, u32 kind, CovCall c, bool dev) {
    if (min_occ < 2) TC_FAIL(ctx, TC_ERR_ARG, "min_occ is at least 2");
    if (kind != TC_COVER_ALL && kind != TC_COVER_LATER) TC_FAIL(ctx, TC_ERR_ARG, "kind is TC_COVER_ALL or TC_COVER_LATER");
    if (n && !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    cov_validate(ctx, c, text, n, min_len);
    if (n == 0 || min_len > n) {
        cov_nothing_covered(ctx, c, text, n, dev);
        return;
    }
    const bool later = kind == TC_COVER_LATER, search = later || min_occ > 2;
    u32 *d_start = c.span_start, *d_slen = c.span_len;
    u8 *d_out = c.out;
    const u64 slots = c.cap < n ? c.cap : n;
    CovWork W;
    esa_plan(ctx, W, text, n, dev,
             [&](Arena &A) {
                 if (dev) return;
                 if (c.what == COV_SPANS && !c.sizes_only) {
                     d_start = A.get<u32>(slots + 1);
                     d_slen = A.get<u32>(slots + 1);
                 } else if (c.what == COV_MASK) {
                     d_out = A.get<u8>(n + 16);
                 } else if (c.what == COV_DEDUP && !c.sizes_only) {
                     d_out = A.get<u8>(slots + 16);
                 }
             },
             [&](Arena &A) { W.carve(ctx, A, n, search, later); });
    const u64 N = n + 1;
    tc_memset_async(ctx, W.len, 0, n * sizeof(u32));
    if (search) W.tree.build(ctx, W.d_lcp, W.lcp_min);
    if (later) {
        W.tree.build(ctx, W.d_sa, W.sa_min);
        cov_seed_kernel<true><<<tc_cdiv(N, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>(W.d_sa, W.d_lcp, W.sa_min, W.lcp_min, (u32)N, W.tree.lf, min_len,
                                                                                 min_occ, W.len);
    } else {
        cov_seed_kernel<false><<<tc_cdiv(N, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>(W.d_sa, W.d_lcp, nullptr, W.lcp_min, (u32)N, W.tree.lf, min_len,
                                                                                  min_occ, W.len);
    }
    TC_LAUNCH_CHECK(ctx);
    cov_finish(ctx, W.core, W.len, W.d_text, n, min_len, c, d_start, d_slen, d_out, dev);
}

// tc_cover_spans_dev, tc_cover_mask_dev, tc_cover_dedup_dev: the cover of a caller's array of lengths
static void cover_entry(tc_ctx *ctx, const u32 *d_len, const u8 *d_text, u64 n, u32 min_len, CovCall c) {
    if (n && !d_len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    cov_validate(ctx, c, d_text, n, min_len);
    if (n == 0) return;
    CovCore C;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { C.carve(A, n); });
    cov_finish(ctx, C, d_len, d_text, n, min_len, c, c.span_start, c.span_len, c.out, true);
}
