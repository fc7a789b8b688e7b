// tc_tr_host.hpp -- host side of the runs / tandem repeats of a text (tc_tr.hpp has the kernels and the method): scratch,
// the launch sequence, and the body of tc_tandem_repeats / tc_tandem_repeats_dev.  Included by textcomp.hip after
// tc_esa_plan.hpp, whose lower layer (esa_sort: the sort, then the LCP scratch over its dead buffers) it runs twice behind
// one mark: once for the text, once for its reverse.
#pragma once
#include "tc_tr.hpp"

// What one call holds in the workspace.  Ahead of the overlay mark, because both sorts must leave it alone: the text
// (host form) and its reverse, one suffix array (dead after each scatter, so the second sort writes it again), isa, comp
// = N - 1 - isa, lcp, isa_r, lcp_r, and the four min trees.  Behind the mark, one after another over the same bytes: the
// first sort's buffers, the first LCP's, the second sort's, the second LCP's, and then the candidate words (2 per
// position: 4 bytes of start, 8 of period and length), the per-start counts and their scan.  Behind the sorts that is
// 2 (the two texts) + 4 (sa) + 5 x 4 (isa, comp, lcp, isa_r, lcp_r) + 24 (candidates) + 8 (counts) + 8 (segment starts) =
// 66 bytes per text byte, plus the four trees (16 / (f - 1)); the sort's own need behind 26 of those bytes where that is
// larger.
struct TrWork {
    u8 *d_text = nullptr, *d_rtext = nullptr;
    u32 *d_sa = nullptr;
    u32 *isa = nullptr, *comp = nullptr, *lcp = nullptr, *isa_r = nullptr, *lcp_r = nullptr;
    MinTree tree;
    u32 *isa_min = nullptr, *comp_min = nullptr, *lcp_min = nullptr, *lcp_r_min = nullptr;
    LcpScratch lcp_ws;
    u32 *c_start = nullptr;     // 2 n entries
    u64 *c_pl = nullptr;        // 2 n entries
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;   // n entries each, and the scan's tile sums
    // everything both sorts leave alone
    void carve_kept(const tc_ctx *ctx, Arena &A, u64 n, bool dry) {
        const u64 N = n + 1;
        d_rtext = A.get<u8>(n + 16);
        d_sa = esa_sa_arg(A.get<u32>(N), dry);
        isa = A.get<u32>(N);
        comp = A.get<u32>(N);
        lcp = A.get<u32>(N);
        isa_r = A.get<u32>(N);
        lcp_r = A.get<u32>(N);
        tree.shape(ctx, (u32)N);
        isa_min = A.get<u32>(tree.words);
        comp_min = A.get<u32>(tree.words);
        lcp_min = A.get<u32>(tree.words);
        lcp_r_min = A.get<u32>(tree.words);
    }
    // what follows the two ESAs, over their dead buffers
    void carve_cand(Arena &A, u64 n) {
        c_start = A.get<u32>(2 * n);
        c_pl = A.get<u64>(2 * n);
        cnt = A.get<u64>(n);
        offs = A.get<u64>(n);
        tsum = A.get<u64>(tc_cdiv(n, SCAN_TILE) + 2);
    }
};

// sort + LCP array of one text of n bytes behind `mark`, then isa (and comp) by scatter: W.d_sa is dead afterwards
static void tr_esa(tc_ctx *ctx, TrWork &W, Arena &A, size_t mark, const u8 *d_text, u64 n, u32 *d_lcp, u32 *d_isa, u32 *d_comp) {
    const u64 N = n + 1;
    A.rewind(mark);
    esa_sort(ctx, A, d_text, n, W.d_sa, W.lcp_ws, false);
    lcp_device(ctx, W.lcp_ws, d_text, n, W.d_sa, d_lcp);
    tr_isa_kernel<<<tc_cdiv(N, TR_NT), TR_NT, 0, ctx->stream>>>(W.d_sa, (u32)N, d_isa, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    if (d_comp) {
        tr_comp_kernel<<<tc_cdiv(N, TR_NT), TR_NT, 0, ctx->stream>>>(d_isa, (u32)N, d_comp);
        TC_LAUNCH_CHECK(ctx);
    }
}

// tc_tandem_repeats, tc_tandem_repeats_dev.  run_start = run_len = run_period = null with capacity 0 is the sizes-only form.
static void tandem_repeats_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 min_period, u32 max_period, u32 min_copies, u32 min_len,
                                 u32 *run_start, u32 *run_len, u32 *run_period, u64 *nrun, bool dev) {
    if (n > TC_MAX_N || !nrun) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nrun;
    *nrun = 0;
    if (min_period == 0 || (max_period != 0 && max_period < min_period))
        TC_FAIL(ctx, TC_ERR_ARG, "min_period is at least 1; max_period is 0 (no limit) or at least min_period");
    if (min_copies < 2 || min_len == 0) TC_FAIL(ctx, TC_ERR_ARG, "min_copies is at least 2, min_len at least 1");
    const bool sizes_only = !run_start && !run_len && !run_period && cap == 0;
    if (!sizes_only && (!run_start || !run_len || !run_period)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (n == 0) return;
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    TrWork W;
    u32 *d_start = run_start, *d_len = run_len, *d_period = run_period;
    const u64 slots = cap < n ? cap : n;        // (a text of n bytes has fewer than n runs)
    size_t mark = 0;
    auto kept = [&](Arena &A, bool dry) {
        W.d_text = dev ? const_cast<u8 *>(text) : A.get<u8>(n + 16);
        W.carve_kept(ctx, A, n, dry);
        if (!dev && !sizes_only) {
            d_start = A.get<u32>(slots + 1);
            d_len = A.get<u32>(slots + 1);
            d_period = A.get<u32>(slots + 1);
        }
        mark = A.off;
    };
    {   // the three overlays behind the mark: a sort, an LCP array, the candidates
        Arena dry(nullptr);
        kept(dry, true);
        esa_sort(ctx, dry, W.d_text, n, W.d_sa, W.lcp_ws, true);
        dry.rewind(mark);
        W.carve_cand(dry, n);
        tc_ws_reserve(ctx, dry.peak);
    }
    if (!dev) esa_fill_text(ctx, text, n, nullptr, 0, false);
    Arena A(ctx->ws);
    kept(A, false);
    hipStream_t s = ctx->stream;
    tr_reverse_kernel<<<tc_cdiv(n, TR_NT), TR_NT, 0, s>>>(W.d_text, (u32)n, W.d_rtext);
    TC_LAUNCH_CHECK(ctx);
    tr_esa(ctx, W, A, mark, W.d_text, n, W.lcp, W.isa, W.comp);
    tr_esa(ctx, W, A, mark, W.d_rtext, n, W.lcp_r, W.isa_r, nullptr);
    A.rewind(mark);
    W.carve_cand(A, n);
    W.tree.build(ctx, W.isa, W.isa_min);
    W.tree.build(ctx, W.comp, W.comp_min);
    W.tree.build(ctx, W.lcp, W.lcp_min);
    W.tree.build(ctx, W.lcp_r, W.lcp_r_min);
    const TrFilter f{min_period, max_period, min_copies, min_len};
    tr_cand_kernel<<<tc_cdiv(n, FM_MS_NT), FM_MS_NT, 0, s>>>(W.d_text, (u32)n, W.isa, W.isa_min, W.comp, W.comp_min, W.lcp, W.lcp_min,
                                                            W.isa_r, W.lcp_r, W.lcp_r_min, W.tree.lf, f, W.c_start, W.c_pl);
    TC_LAUNCH_CHECK(ctx);
    const u32 cgrid = tc_cdiv(2 * n, TR_NT);
    tc_memset_async(ctx, W.cnt, 0, n * sizeof(u64));
    tr_count_kernel<<<cgrid, TR_NT, 0, s>>>(W.c_start, W.c_pl, 2 * n, (u32)n, W.cnt);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, W.cnt, n, W.tsum, W.offs, cap, sizes_only, nrun, "run");
    if (!sizes_only && need) {
        tr_fill_kernel<<<cgrid, TR_NT, 0, s>>>(W.c_start, W.c_pl, 2 * n, (u32)n, W.cnt, W.offs, need, d_start, d_len, d_period);
        TC_LAUNCH_CHECK(ctx);
        tr_order_kernel<<<tc_cdiv(n, TR_NT), TR_NT, 0, s>>>(W.offs, (u32)n, need, d_len, d_period);
        TC_LAUNCH_CHECK(ctx);
        if (!dev) {
            tc_d2h(ctx, run_start, d_start, need * sizeof(u32));
            tc_d2h(ctx, run_len, d_len, need * sizeof(u32));
            tc_d2h(ctx, run_period, d_period, need * sizeof(u32));
        }
    }
    tc_sync_check(ctx);
}
