// tc_lcp_host.hpp -- host side of the LCP array (tc_lcp.hpp has the kernels and the algorithm): scratch, the launch
// sequence, and the bodies of tc_suffix_array_dev / tc_lcp_array_dev / tc_lcp_summary_dev (tc_lcp_array, which sorts first, is
// in tc_esa_plan.hpp).  Included by tc_fm_host.hpp (lcp_device makes the LCP part of an index) and textcomp.hip, after
// tc_encode_host.hpp (sa_build, the copy helpers).
#pragma once
#include "tc_lcp.hpp"

// the short cap of this context: TC_LCP_SHORT_CAP unless the debug interface set another (tc_dbg_lcp_set_short_cap)
static u32 lcp_short_cap(const tc_ctx *ctx) { return ctx->lcp_cap ? ctx->lcp_cap : TC_LCP_SHORT_CAP; }
// slots of the long-item list: the irreducible values sum to at most 2 n log2 n, so at most that over `cap` of them
// reach the cap -- and never more than there are positions
static u64 lcp_list_cap(u64 n, u32 cap) {
    const u64 bound = 2 * n * (u64)ceil_log2_u64(n + 1) / cap + 1;
    return bound < n ? bound : n;
}

struct LcpScratch {
    u32 *v = nullptr;       // N words: phi, then V, then its scan
    u32 *list = nullptr;    // long items
    u32 *tmax = nullptr;    // one word per scan tile
    u32 *count = nullptr;   // long items drawn
    u64 list_cap = 0;
    u32 ntiles = 0, cap = 0;
    void carve(const tc_ctx *ctx, Arena &A, u64 n) {
        const u64 N = n + 1;
        cap = lcp_short_cap(ctx);
        list_cap = lcp_list_cap(n, cap);
        ntiles = tc_cdiv(N, LCP_SCAN_TILE);
        v = A.get<u32>(N);
        list = A.get<u32>(list_cap);
        tmax = A.get<u32>(ntiles);
        count = A.get<u32>(1);
    }
};

// d_lcp[0 .. n] from d_text[0 .. n) and d_sa[0 .. n], n >= 1: the five steps, on the context's stream.  The caller
// synchronises (tc_sync_check turns LCP_ERR_SA into TC_ERR_MALFORMED).
static void lcp_device(tc_ctx *ctx, const LcpScratch &W, const u8 *d_text, u64 n, const u32 *d_sa, u32 *d_lcp) {
    hipStream_t s = ctx->stream;
    const u64 N = n + 1;
    const u32 grid = tc_cdiv(N, LCP_NT);
    tc_memset_async(ctx, W.v, 0xff, N * sizeof(u32));
    tc_memset_async(ctx, W.count, 0, sizeof(u32));
    lcp_phi_kernel<<<grid, LCP_NT, 0, s>>>(d_sa, N, (u32)n, W.v, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    lcp_irreducible_kernel<<<grid, LCP_NT, 0, s>>>(d_text, (u32)n, d_sa, W.v, W.cap, W.list, (u32)W.list_cap, W.count, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    // (the number of long items stays on the device: a grid that fills it, every workgroup reads the count)
    const u64 want = W.list_cap < (u64)tc_persistent_grid(ctx, 8) ? W.list_cap : (u64)tc_persistent_grid(ctx, 8);
    lcp_long_kernel<<<(u32)(want ? want : 1), LCP_NT, 0, s>>>(d_text, (u32)n, W.v, W.cap, W.list, (u32)W.list_cap, W.count);
    TC_LAUNCH_CHECK(ctx);
    lcp_scan_reduce_kernel<<<W.ntiles, LCP_SCAN_NT, 0, s>>>(W.v, N, W.tmax);
    TC_LAUNCH_CHECK(ctx);
    lcp_scan_tiles_kernel<<<1, LCP_SCAN_NT, 0, s>>>(W.tmax, W.ntiles, tc_cdiv(W.ntiles, LCP_SCAN_NT));
    TC_LAUNCH_CHECK(ctx);
    lcp_scan_apply_kernel<<<W.ntiles, LCP_SCAN_NT, 0, s>>>(W.v, N, W.tmax);
    TC_LAUNCH_CHECK(ctx);
    lcp_gather_kernel<<<grid, LCP_NT, 0, s>>>(d_sa, N, (u32)n, W.v, d_lcp);
    TC_LAUNCH_CHECK(ctx);
}

// tc_suffix_array_dev: sa_build into the caller's array (the last column it also makes goes to the workspace)
static void suffix_array_dev_entry(tc_ctx *ctx, const u8 *d_text, u64 n, u32 *d_sa) {
    if (n > TC_MAX_N || !d_sa) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) {   // as tc_suffix_array: one row, 0
        tc_memset_async(ctx, d_sa, 0, sizeof(u32));
        tc_sync_check(ctx);
        return;
    }
    if (!d_text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = n + 1;
    u64 primary = 0;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool dry) {
        u8 *d_L = A.get<u8>(n + 1 + 16);
        sa_build(ctx, A, d_text, n, d_sa, d_L, &primary, nullptr, dry);
    });
    tc_sync_check(ctx);
}

// tc_lcp_array_dev
static void lcp_array_dev_entry(tc_ctx *ctx, const u8 *d_text, u64 n, const u32 *d_sa, u32 *d_lcp) {
    if (n > TC_MAX_N || !d_sa || !d_lcp) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) {   // one row (d_sa is not read)
        tc_memset_async(ctx, d_lcp, 0, sizeof(u32));
        tc_sync_check(ctx);
        return;
    }
    if (!d_text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    LcpScratch W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { W.carve(ctx, A, n); });
    lcp_device(ctx, W, d_text, n, d_sa, d_lcp);
    tc_sync_check(ctx);
}

// tc_lcp_summary_dev
static void lcp_summary_entry(tc_ctx *ctx, const u32 *d_lcp, u64 N, u32 *max_lcp, u64 *row, u64 *sum) {
    if (!d_lcp || N == 0 || N > TC_MAX_N + 1 || !max_lcp || !row || !sum) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    u64 *d_out = nullptr;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { d_out = A.get<u64>(2); });
    tc_memset_async(ctx, d_out, 0, 2 * sizeof(u64));
    const u32 full = tc_cdiv(N, LCP_NT), most = tc_persistent_grid(ctx, 8);
    lcp_summary_kernel<<<full < most ? full : most, LCP_NT, 0, ctx->stream>>>(d_lcp, N, d_out);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[8], d_out, 2 * sizeof(u64));
    tc_sync_check(ctx);
    const u64 key = ctx->h_scalars[8];
    *max_lcp = (u32)(key >> 32);
    *row = (u64)(0xffffffffu - (u32)key);
    *sum = ctx->h_scalars[9];
}
