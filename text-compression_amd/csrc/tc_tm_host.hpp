// tc_tm_host.hpp -- host side of the comparison of two texts (tc_tm.hpp has the kernels and the method): scratch, the
// launch sequence, and the bodies of tc_text_match_stats / tc_text_mems / tc_text_lcs, their _dev forms and
// tc_mems_from_stats_dev.  Included by textcomp.hip after tc_esa_plan.hpp (the ESA is esa_plan's, over the two texts copied
// into one) and tc_lcp_host.hpp, whose summary kernel is the LCS reduction.
#pragma once
#include "tc_tm.hpp"

// the scratch of the MEM filter over a positions: 16 bytes per tile of TM_TILE positions and the scan's sums
struct TmMemWork {
    u32 ntiles = 0;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    void carve(Arena &A, u64 a) {
        ntiles = tc_cdiv(a, TM_TILE);
        cnt = A.get<u64>(ntiles);
        offs = A.get<u64>(ntiles + 1);
        tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
    }
};

// What one call holds in the workspace, n = a + b: the text Q T, its enhanced suffix array and the results the caller did
// not give in HBM ahead of the overlay mark, and -- over the sort's and then the LCP's dead buffers -- the min tree of
// the LCP array, the T-row flags (the two row lists later: the flags are dead once scanned) and their scan.  Behind the
// sort that is 1 (text) + 4 (sa) + 4 (lcp) + 8 (flags / trow, qrow) + 8 (cnt) = 25 bytes per byte of the two texts, plus
// the tree (4 / (f - 1)), up to 12 per query byte for the three results and 16 bytes per tile of the MEM filter; the
// sort's own need where that is larger.
struct TmWork : Esa {
    u32 *d_len = nullptr, *d_pos = nullptr, *d_occ = nullptr;   // a entries each; pos and occ may stay null
    MinTree tree;
    u32 *lcp_min = nullptr;
    u64 *flag = nullptr;    // N + 1 entries; then trow (b words) and qrow (a words)
    u64 *cnt = nullptr;     // N + 1 entries
    u64 *csum = nullptr;    // the scan's tile sums
    u64 *red = nullptr;     // the LCS reduction's two words, then the (len, pos) of the one position it reports
    TmMemWork mem;
    void carve(const tc_ctx *ctx, Arena &A, u64 a, u64 b) {
        const u64 N = a + b + 1;
        tree.shape(ctx, (u32)N);
        lcp_min = A.get<u32>(tree.words);
        flag = A.get<u64>(N + 1);
        cnt = A.get<u64>(N + 1);
        csum = A.get<u64>(tc_cdiv(N + 1, SCAN_TILE) + 2);
        red = A.get<u64>(2);
        mem.carve(A, a);
    }
    u32 *trow() const { return reinterpret_cast<u32 *>(flag); }
    u32 *qrow(u64 b) const { return reinterpret_cast<u32 *>(flag) + b; }
};

// The matching statistics of query against target, a >= 1, b >= 1, a + b <= TC_MAX_N, on the context's stream: W.d_len
// (and W.d_pos, W.d_occ where they are not null) hold them afterwards.  The two texts -- device pointers (dev) or host
// pointers -- are copied into one workspace text, the workspace's first carve; outputs(A) carves what the call keeps
// besides, ahead of everything that is overlaid, and sets W.d_len / d_pos / d_occ.
template <class F>
static void tm_stats_device(tc_ctx *ctx, TmWork &W, const u8 *query, u64 a, const u8 *target, u64 b, bool dev, F &&outputs) {
    const u64 n = a + b, N = n + 1;
    EsaOpts o;
    o.text2 = target;
    o.n2 = b;
    esa_plan(ctx, W, query, a, dev, outputs, [&](Arena &A) { W.carve(ctx, A, a, b); }, o);
    hipStream_t s = ctx->stream;
    W.tree.build(ctx, W.d_lcp, W.lcp_min);
    tm_flag_kernel<<<tc_cdiv(N + 1, 256), 256, 0, s>>>(W.d_sa, (u32)N, (u32)a, (u32)n, W.flag);
    TC_LAUNCH_CHECK(ctx);
    tc_scan64(ctx, W.flag, N + 1, W.csum, W.cnt);
    tm_compact_kernel<<<tc_cdiv(n, 256), 256, 0, s>>>(W.d_sa, (u32)N, (u32)a, (u32)n, W.cnt, W.trow(), W.qrow(b));
    TC_LAUNCH_CHECK(ctx);
    const u32 grid = tc_cdiv(a, FM_MS_NT);
    if (W.d_pos || W.d_occ)
        tm_row_kernel<true><<<grid, FM_MS_NT, 0, s>>>(W.d_sa, W.d_lcp, W.lcp_min, (u32)N, W.tree.lf, W.cnt, W.trow(), W.qrow(b), (u32)a, (u32)b,
                                                     TM_ALL, W.d_len, W.d_pos, W.d_occ);
    else
        tm_row_kernel<false><<<grid, FM_MS_NT, 0, s>>>(W.d_sa, W.d_lcp, W.lcp_min, (u32)N, W.tree.lf, W.cnt, W.trow(), W.qrow(b), (u32)a, (u32)b,
                                                      TM_ALL, W.d_len, nullptr, nullptr);
    TC_LAUNCH_CHECK(ctx);
}

static void tm_check_sizes(tc_ctx *ctx, u64 a, u64 b) {
    if (a > TC_MAX_N || b > TC_MAX_N || a + b > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "the two texts hold more than TC_MAX_N bytes");
}

// tc_text_match_stats, tc_text_match_stats_dev
static void text_match_stats_entry(tc_ctx *ctx, const u8 *query, u64 a, const u8 *target, u64 b, u32 *ms_len, u32 *ms_pos,
                                   u32 *ms_occ, bool dev) {
    if (!ms_len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    tm_check_sizes(ctx, a, b);
    if (a == 0) return;
    if (!query || (b && !target)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (b == 0) {       // nothing occurs in the empty text: zeros, without a sort
        u32 *const out[3] = {ms_len, ms_pos, ms_occ};
        for (u32 *p : out) {
            if (!p) continue;
            if (dev) tc_memset_async(ctx, p, 0, a * sizeof(u32));
            else memset(p, 0, a * sizeof(u32));
        }
        if (dev) tc_sync_check(ctx);
        return;
    }
    TmWork W;
    tm_stats_device(ctx, W, query, a, target, b, dev, [&](Arena &A) {
        W.d_len = dev ? ms_len : A.get<u32>(a);
        W.d_pos = !ms_pos ? nullptr : dev ? ms_pos : A.get<u32>(a);
        W.d_occ = !ms_occ ? nullptr : dev ? ms_occ : A.get<u32>(a);
    });
    if (!dev) {
        tc_d2h(ctx, ms_len, W.d_len, a * sizeof(u32));
        if (ms_pos) tc_d2h(ctx, ms_pos, W.d_pos, a * sizeof(u32));
        if (ms_occ) tc_d2h(ctx, ms_occ, W.d_occ, a * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// The MEM filter over d_len / d_pos (a >= 1 entries, in HBM) on the context's stream: the count (the host waits for it),
// and -- unless sizes_only -- the fill.  Returns the count; a capacity that is too small throws after *nmem is set.
static u64 tm_mems_filter(tc_ctx *ctx, const TmMemWork &M, const u32 *d_len, const u32 *d_pos, u64 a, u32 min_len, u32 *d_start,
                          u32 *d_mpos, u32 *d_mlen, u64 cap, bool sizes_only, u64 *nmem) {
    hipStream_t s = ctx->stream;
    tm_mem_count_kernel<<<M.ntiles, TM_NT, 0, s>>>(d_len, a, min_len, M.cnt);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, M.cnt, M.ntiles, M.tsum, M.offs, cap, sizes_only, nmem, "MEM");
    if (sizes_only || need == 0) return need;
    tm_mem_fill_kernel<<<M.ntiles, TM_NT, 0, s>>>(d_len, d_pos, a, min_len, M.offs, need, d_start, d_mpos, d_mlen);
    TC_LAUNCH_CHECK(ctx);
    return need;
}

// what the three MEM calls check before anything else; *nmem is untouched where this fails
static bool tm_mems_args(tc_ctx *ctx, u32 min_len, const u32 *mem_start, const u32 *mem_pos, const u32 *mem_len, const u64 *nmem) {
    if (!nmem) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (min_len == 0) TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 1");
    const bool sizes_only = !mem_start && !mem_pos && !mem_len && *nmem == 0;
    if (!sizes_only && (!mem_start || !mem_pos || !mem_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    return sizes_only;
}

// tc_mems_from_stats_dev
static void mems_from_stats_entry(tc_ctx *ctx, const u32 *d_ms_len, const u32 *d_ms_pos, u64 a, u32 min_len, u32 *d_mem_start,
                                  u32 *d_mem_pos, u32 *d_mem_len, u64 *nmem) {
    const bool sizes_only = tm_mems_args(ctx, min_len, d_mem_start, d_mem_pos, d_mem_len, nmem);
    if (a > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "more than TC_MAX_N positions");
    const u64 cap = *nmem;
    if (a == 0) {
        *nmem = 0;
        return;
    }
    if (!d_ms_len || (!sizes_only && !d_ms_pos)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    *nmem = 0;
    TmMemWork M;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { M.carve(A, a); });
    tm_mems_filter(ctx, M, d_ms_len, d_ms_pos, a, min_len, d_mem_start, d_mem_pos, d_mem_len, cap, sizes_only, nmem);
    tc_sync_check(ctx);
}

// tc_text_mems, tc_text_mems_dev.  mem_start = mem_pos = mem_len = null with capacity 0 is the sizes-only form.
static void text_mems_entry(tc_ctx *ctx, const u8 *query, u64 a, const u8 *target, u64 b, u32 min_len, u32 *mem_start, u32 *mem_pos,
                            u32 *mem_len, u64 *nmem, bool dev) {
    const bool sizes_only = tm_mems_args(ctx, min_len, mem_start, mem_pos, mem_len, nmem);
    tm_check_sizes(ctx, a, b);
    const u64 cap = *nmem;
    if (a && (!query || (b && !target))) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    *nmem = 0;
    if (a == 0 || b == 0) return;       // (no byte of the query occurs in the empty text: no MEM)
    TmWork W;
    u32 *d_start = mem_start, *d_mpos = mem_pos, *d_mlen = mem_len;
    const u64 slots = cap < a ? cap : a;        // (at most one MEM starts at a position)
    tm_stats_device(ctx, W, query, a, target, b, dev, [&](Arena &A) {
        W.d_len = A.get<u32>(a);
        W.d_pos = sizes_only ? nullptr : A.get<u32>(a);
        if (dev || sizes_only) return;
        d_start = A.get<u32>(slots + 1);
        d_mpos = A.get<u32>(slots + 1);
        d_mlen = A.get<u32>(slots + 1);
    });
    const u64 need = tm_mems_filter(ctx, W.mem, W.d_len, W.d_pos, a, min_len, d_start, d_mpos, d_mlen, cap, sizes_only, nmem);
    if (!dev && !sizes_only && need) {
        tc_d2h(ctx, mem_start, d_start, need * sizeof(u32));
        tc_d2h(ctx, mem_pos, d_mpos, need * sizeof(u32));
        tc_d2h(ctx, mem_len, d_mlen, need * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// tc_text_lcs, tc_text_lcs_dev: the four results are host words in both forms.  ms_len alone is computed (the row kernel
// without its searches); the reduction is the one of tc_lcp_summary_dev over it: the largest value, of its positions the
// smallest, and the sum; then the row kernel once more for that one position's ms_pos.
static void text_lcs_entry(tc_ctx *ctx, const u8 *query, u64 a, const u8 *target, u64 b, u32 *len, u64 *qpos, u64 *tpos, u64 *sum,
                           bool dev) {
    if (!len || !qpos || !tpos || !sum) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    tm_check_sizes(ctx, a, b);
    if (a && (!query || (b && !target))) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    *len = 0; *qpos = 0; *tpos = 0; *sum = 0;
    if (a == 0 || b == 0) return;
    TmWork W;
    tm_stats_device(ctx, W, query, a, target, b, dev, [&](Arena &A) { W.d_len = A.get<u32>(a); });
    hipStream_t s = ctx->stream;
    tc_memset_async(ctx, W.red, 0, 2 * sizeof(u64));
    const u32 full = tc_cdiv(a, LCP_NT), most = tc_persistent_grid(ctx, 8);
    lcp_summary_kernel<<<full < most ? full : most, LCP_NT, 0, s>>>(W.d_len, a, W.red);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[8], W.red, 2 * sizeof(u64));
    tc_sync_check(ctx);
    const u64 key = ctx->h_scalars[8];
    const u32 best = (u32)(key >> 32);
    const u64 at = (u64)(0xffffffffu - (u32)key);
    *sum = ctx->h_scalars[9];
    if (best == 0 || at >= a) return;
    u32 *one = reinterpret_cast<u32 *>(W.red);
    tm_row_kernel<true><<<tc_cdiv(a, FM_MS_NT), FM_MS_NT, 0, s>>>(W.d_sa, W.d_lcp, W.lcp_min, (u32)(a + b + 1), W.tree.lf, W.cnt, W.trow(), W.qrow(b),
                                                                (u32)a, (u32)b, (u32)at, one, one + 1, nullptr);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[10], one + 1, sizeof(u32));
    tc_sync_check(ctx);
    *len = best;
    *qpos = at;
    *tpos = (u32)ctx->h_scalars[10];
}
