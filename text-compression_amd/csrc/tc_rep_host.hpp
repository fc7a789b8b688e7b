// tc_rep_host.hpp -- host side of the maximal / supermaximal repeats (tc_rep.hpp has the kernels and the definitions):
// scratch, the launch sequence, and the body of tc_repeats / tc_repeats_dev.  Included by textcomp.hip after
// tc_lz_host.hpp, whose ESA plan (sa_build, then lcp_device over the sort's dead buffers) and lz_build_tree it follows.
#pragma once
#include "tc_rep.hpp"

// What one call holds in the workspace: the text (host form), the enhanced suffix array and the last column ahead of
// the overlay mark, and -- over the sort's and then the LCP's dead buffers -- the min tree of the LCP array, the
// left-context flags (the packed rows later: the flags are dead once scanned), their scan and the tiles' counts.
// Behind the sort that is 4 (sa) + 4 (lcp) + 1 (last column) + 8 (flags / packed rows) + 8 (chg) = 25 bytes per text
// byte, plus the tree (4 / (f - 1)) and 16 bytes per tile of REP_TILE rows; the sort's own need where that is larger.
struct RepWork {
    u8 *d_text = nullptr, *d_L = nullptr;
    u32 *d_sa = nullptr, *d_lcp = nullptr;
    LcpScratch lcp_ws;
    u32 lf = 0, tree_levels = 0, tree_words = 0;
    u32 tree_off[FM_MS_MAXLEV + 1], tree_cnt[FM_MS_MAXLEV + 1];
    u32 *lcp_min = nullptr;
    u64 *pack = nullptr;    // N entries: the flags, then occ << 32 | lb of every row
    u64 *chg = nullptr;     // N entries
    u64 *csum = nullptr;    // the scan's tile sums
    u32 ntiles = 0;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    void carve(const tc_ctx *ctx, Arena &A, u64 n) {
        const u64 N = n + 1;
        lf = fm_log2(ctx->fm_lcp_fanout ? ctx->fm_lcp_fanout : FM_LCP_FANOUT);
        tree_levels = fm_ms_tree_shape((u32)N, lf, tree_off, tree_cnt, &tree_words);
        lcp_min = A.get<u32>(tree_words);
        pack = A.get<u64>(N);
        chg = A.get<u64>(N);
        csum = A.get<u64>(tc_cdiv(N, SCAN_TILE) + 2);
        ntiles = tc_cdiv(N, REP_TILE);
        cnt = A.get<u64>(ntiles);
        offs = A.get<u64>(ntiles + 1);
        tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
    }
};

// tc_repeats, tc_repeats_dev.  rep_pos = rep_len = rep_occ = null with capacity 0 is the sizes-only form.
static void repeats_entry(tc_ctx *ctx, const u8 *text, u64 n, int kind, u32 min_len, u32 min_occ, u32 *sa, u32 *rep_pos,
                          u32 *rep_len, u32 *rep_occ, u32 *rep_row, u64 *nrep, bool dev) {
    if (n > TC_MAX_N || !nrep) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nrep;
    *nrep = 0;
    if (kind != TC_REPEAT_MAXIMAL && kind != TC_REPEAT_SUPERMAXIMAL) TC_FAIL(ctx, TC_ERR_ARG, "kind is TC_REPEAT_MAXIMAL or TC_REPEAT_SUPERMAXIMAL");
    if (min_len == 0 || min_occ < 2) TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 1, min_occ at least 2");
    const bool sizes_only = !rep_pos && !rep_len && !rep_occ && cap == 0;
    if (!sizes_only && (!rep_pos || !rep_len || !rep_occ)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (n == 0) {       // one row, 0, as tc_suffix_array
        if (sa && dev) {
            tc_memset_async(ctx, sa, 0, sizeof(u32));
            tc_sync_check(ctx);
        } else if (sa) {
            sa[0] = 0;
        }
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    RepWork W;
    u32 *d_pos = rep_pos, *d_len = rep_len, *d_occ = rep_occ, *d_row = rep_row;
    const u64 slots = cap < n ? cap : n;        // (a text of n bytes has fewer than n maximal repeats)
    u64 primary = 0;
    auto plan = [&](Arena &A, bool dry) {
        W.d_text = dev ? const_cast<u8 *>(text) : A.get<u8>(n + 16);
        u32 *p = dev && sa ? sa : A.get<u32>(N);    // (a dry run carves without a base: any non-null value tells sa_build that the array is provided)
        W.d_sa = dry ? reinterpret_cast<u32 *>(sizeof(u32)) : p;
        W.d_lcp = A.get<u32>(N);
        W.d_L = A.get<u8>(N + 16);                  // ahead of the mark: the last column outlives the sort
        if (!dev && !sizes_only) {
            d_pos = A.get<u32>(slots + 1);
            d_len = A.get<u32>(slots + 1);
            d_occ = A.get<u32>(slots + 1);
            if (rep_row) d_row = A.get<u32>(slots + 1);
        }
        const size_t mark = A.off;
        sa_build(ctx, A, W.d_text, n, W.d_sa, W.d_L, &primary, nullptr, dry);
        A.rewind(mark);
        W.lcp_ws.carve(ctx, A, n);
        A.rewind(mark);
        W.carve(ctx, A, n);
    };
    Arena dry(nullptr);
    plan(dry, true);
    tc_ws_reserve(ctx, dry.peak);
    if (!dev) {     // the text is the first carve: upload it between the reserve and the run, as lcp_array_host_entry does
        Arena A0(ctx->ws);
        tc_h2d(ctx, A0.get<u8>(n + 16), text, n);
    }
    Arena A(ctx->ws);
    plan(A, false);
    hipStream_t s = ctx->stream;
    lcp_device(ctx, W.lcp_ws, W.d_text, n, W.d_sa, W.d_lcp);
    lz_build_tree(ctx, W, W.d_lcp, W.lcp_min);
    const u32 rows = tc_cdiv(N, 256);
    rep_left_kernel<<<rows, 256, 0, s>>>(W.d_L, (u32)N, (u32)primary, W.pack);
    TC_LAUNCH_CHECK(ctx);
    tc_scan64(ctx, W.pack, N, W.csum, W.chg);
    if (kind == TC_REPEAT_SUPERMAXIMAL)
        rep_row_kernel<true><<<rows, FM_MS_NT, 0, s>>>(W.d_lcp, W.lcp_min, (u32)N, W.lf, W.chg, W.d_L, (u32)primary, min_len, min_occ, W.pack);
    else
        rep_row_kernel<false><<<rows, FM_MS_NT, 0, s>>>(W.d_lcp, W.lcp_min, (u32)N, W.lf, W.chg, W.d_L, (u32)primary, min_len, min_occ, W.pack);
    TC_LAUNCH_CHECK(ctx);
    rep_count_kernel<<<W.ntiles, REP_NT, 0, s>>>(W.pack, (u32)N, W.cnt);
    TC_LAUNCH_CHECK(ctx);
    const u64 *d_total = tc_scan64(ctx, W.cnt, W.ntiles, W.tsum, W.offs);
    tc_d2h(ctx, &ctx->h_scalars[9], d_total, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    const u64 need = ctx->h_scalars[9];
    *nrep = need;
    if (need > cap && !sizes_only) {
        tc_sync_check(ctx);
        TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu repeat slots, have %llu", (unsigned long long)need, (unsigned long long)cap);
    }
    if (!sizes_only && need) {
        rep_fill_kernel<<<W.ntiles, REP_NT, 0, s>>>(W.pack, (u32)N, W.offs, W.d_sa, W.d_lcp, d_pos, d_len, d_occ, d_row);
        TC_LAUNCH_CHECK(ctx);
        if (!dev) {
            tc_d2h(ctx, rep_pos, d_pos, need * sizeof(u32));
            tc_d2h(ctx, rep_len, d_len, need * sizeof(u32));
            tc_d2h(ctx, rep_occ, d_occ, need * sizeof(u32));
            if (rep_row) tc_d2h(ctx, rep_row, d_row, need * sizeof(u32));
        }
    }
    if (!dev && sa) tc_d2h(ctx, sa, W.d_sa, N * sizeof(u32));
    tc_sync_check(ctx);
}
