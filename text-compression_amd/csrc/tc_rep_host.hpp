// tc_rep_host.hpp -- host side of the maximal / supermaximal repeats (tc_rep.hpp has the kernels and the definitions):
// scratch, the launch sequence, and the body of tc_repeats / tc_repeats_dev.  Included by textcomp.hip after
// tc_esa_plan.hpp: the ESA is esa_plan's, with the caller's sa (the _dev form) and the last column kept.
#pragma once
#include "tc_rep.hpp"

// What one call holds in the workspace: the text (host form), the enhanced suffix array and the last column ahead of
// the overlay mark, and -- over the sort's and then the LCP's dead buffers -- the min tree of the LCP array, the
// left-context flags (the packed rows later: the flags are dead once scanned), their scan and the tiles' counts.
// Behind the sort that is 4 (sa) + 4 (lcp) + 1 (last column) + 8 (flags / packed rows) + 8 (chg) = 25 bytes per text
// byte, plus the tree (4 / (f - 1)) and 16 bytes per tile of REP_TILE rows; the sort's own need where that is larger.
struct RepWork : Esa {
    MinTree tree;
    u32 *lcp_min = nullptr;
    u64 *pack = nullptr;    // N entries: the flags, then occ << 32 | lb of every row
    u64 *chg = nullptr;     // N entries
    u64 *csum = nullptr;    // the scan's tile sums
    u32 ntiles = 0;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    void carve(const tc_ctx *ctx, Arena &A, u64 n) {
        const u64 N = n + 1;
        tree.shape(ctx, (u32)N);
        lcp_min = A.get<u32>(tree.words);
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
    if (n == 0) {
        esa_empty_sa(ctx, sa, dev);
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    RepWork W;
    u32 *d_pos = rep_pos, *d_len = rep_len, *d_occ = rep_occ, *d_row = rep_row;
    const u64 slots = cap < n ? cap : n;        // (a text of n bytes has fewer than n maximal repeats)
    EsaOpts o;
    o.sa = dev ? sa : nullptr;
    o.keep_L = true;
    esa_plan(ctx, W, text, n, dev,
             [&](Arena &A) {
                 if (!dev && !sizes_only) {
                     d_pos = A.get<u32>(slots + 1);
                     d_len = A.get<u32>(slots + 1);
                     d_occ = A.get<u32>(slots + 1);
                     if (rep_row) d_row = A.get<u32>(slots + 1);
                 }
             },
             [&](Arena &A) { W.carve(ctx, A, n); }, o);
    hipStream_t s = ctx->stream;
    const u32 primary = (u32)W.primary;
    W.tree.build(ctx, W.d_lcp, W.lcp_min);
    const u32 rows = tc_cdiv(N, 256);
    rep_left_kernel<<<rows, 256, 0, s>>>(W.d_L, (u32)N, primary, W.pack);
    TC_LAUNCH_CHECK(ctx);
    tc_scan64(ctx, W.pack, N, W.csum, W.chg);
    if (kind == TC_REPEAT_SUPERMAXIMAL)
        rep_row_kernel<true><<<rows, FM_MS_NT, 0, s>>>(W.d_lcp, W.lcp_min, (u32)N, W.tree.lf, W.chg, W.d_L, primary, min_len, min_occ, W.pack);
    else
        rep_row_kernel<false><<<rows, FM_MS_NT, 0, s>>>(W.d_lcp, W.lcp_min, (u32)N, W.tree.lf, W.chg, W.d_L, primary, min_len, min_occ, W.pack);
    TC_LAUNCH_CHECK(ctx);
    rep_count_kernel<<<W.ntiles, REP_NT, 0, s>>>(W.pack, (u32)N, W.cnt);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, W.cnt, W.ntiles, W.tsum, W.offs, cap, sizes_only, nrep, "repeat");
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
