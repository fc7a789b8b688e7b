// tc_maw_host.hpp -- host side of the minimal absent words (tc_maw.hpp has the kernels and the definitions): scratch, the
// launch sequence, and the bodies of tc_absent_words / tc_absent_words_dev and tc_absent_word_profile /
// tc_absent_word_profile_dev.  Included by textcomp.hip after tc_esa_plan.hpp (the ESA is esa_plan's, with the last column
// kept and the sort's byte counts) and tc_rep_host.hpp (rep_left_kernel).
#pragma once
#include "tc_maw.hpp"

// What one call holds in the workspace: the text (host form), the enhanced suffix array and the last column ahead of the
// overlay mark, and -- over the sort's and then the LCP's dead buffers -- the min tree of the LCP array, the OR tree of the
// last column, the left-context flags (the rows' word counts later: the flags are dead once scanned), their scan and the
// tiles' counts.  Behind the sort that is 4 (sa) + 4 (lcp) + 1 (last column) + 8 (flags / row counts) + 8 (chg) = 25 bytes
// per text byte, plus the min tree (4 / (f - 1)), the OR tree (carved at its wide size, 32 / (f - 1), before the alphabet is
// known; the narrow instance uses a quarter of it) and 16 bytes per tile of FM_MS_NT rows; the sort's own need where that is
// larger.  The list's 9 bytes per word lie ahead of the mark in the host form.
struct MawWork : Esa {
    MinTree tree;
    u32 *lcp_min = nullptr;
    u64 *ortree = nullptr;  // 4 tree.words: level k starts at word tree.off[k] * (wide ? 4 : 1)
    u64 *flag = nullptr;    // N entries: the flags, then (as u32) the word count of every row
    u64 *chg = nullptr;     // N entries
    u64 *csum = nullptr;    // the scan's tile sums
    u32 ntiles = 0;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    u64 *hist = nullptr;    // the profile: kmax + 1 bins and the total
    void carve(const tc_ctx *ctx, Arena &A, u64 n, u32 kmax) {
        const u64 N = n + 1;
        tree.shape(ctx, (u32)N);
        lcp_min = A.get<u32>(tree.words);
        ortree = A.get<u64>(4 * (size_t)tree.words);
        flag = A.get<u64>(N);
        chg = A.get<u64>(N);
        csum = A.get<u64>(tc_cdiv(N, SCAN_TILE) + 2);
        ntiles = tc_cdiv(N, FM_MS_NT);
        if (kmax) {
            hist = A.get<u64>((size_t)kmax + 2);
        } else {
            cnt = A.get<u64>(ntiles);
            offs = A.get<u64>(ntiles + 1);
            tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
        }
    }
};

// The ESA of the text (n >= 1), the two trees and the change counts, on the context's stream; P is filled for the row
// kernels.  outputs(A) carves what a host form returns, ahead of everything that is overlaid.  Returns whether the text
// has more than 64 distinct bytes (the wide instances).
template <class F>
static bool maw_prepare(tc_ctx *ctx, MawWork &W, const u8 *text, u64 n, bool dev, u32 kmax, MawArgs &P, F &&outputs) {
    const u64 N = n + 1;
    u32 counts[256] = {};
    EsaOpts o;
    o.keep_L = true;
    o.counts = counts;
    esa_plan(ctx, W, text, n, dev, outputs, [&](Arena &A) { W.carve(ctx, A, n, kmax); }, o);
    hipStream_t s = ctx->stream;
    const u64 primary = W.primary;
    W.tree.build(ctx, W.d_lcp, W.lcp_min);
    rep_left_kernel<<<tc_cdiv(N, 256), 256, 0, s>>>(W.d_L, (u32)N, (u32)primary, W.flag);
    TC_LAUNCH_CHECK(ctx);
    tc_scan64(ctx, W.flag, N, W.csum, W.chg);
    P.lcp = W.d_lcp; P.lmin = W.lcp_min; P.sa = W.d_sa; P.chg = W.chg; P.L = W.d_L; P.ortree = W.ortree;
    P.N = (u32)N; P.lf = W.tree.lf; P.primary = (u32)primary;
    u32 sigma = 0;
    for (u32 i = 0; i < 4; i++) P.alpha[i] = 0;
    for (u32 v = 0; v < 256; v++) {
        if (!counts[v]) continue;
        P.alpha[v >> 6] |= 1ull << (v & 63u);
        sigma++;
    }
    const bool wide = sigma > 64;
    const u32 words = wide ? 4u : 1u;
    const u64 *src = nullptr;
    for (u32 k = 1; k <= W.tree.levels; k++) {      // the OR tree, level over level: level 1 from the last column
        u64 *dst = W.ortree + (size_t)W.tree.off[k] * words;
        const u32 grid = tc_cdiv(W.tree.cnt[k], 256);
        if (wide) maw_tree_kernel<true><<<grid, 256, 0, s>>>(P, src, W.tree.cnt[k - 1], dst, W.tree.cnt[k]);
        else maw_tree_kernel<false><<<grid, 256, 0, s>>>(P, src, W.tree.cnt[k - 1], dst, W.tree.cnt[k]);
        TC_LAUNCH_CHECK(ctx);
        src = dst;
    }
    return wide;
}

template <int MODE>
static void maw_rows(tc_ctx *ctx, const MawWork &W, const MawArgs &P, bool wide, u64 total, u8 *d_left, u32 *d_pos, u32 *d_len,
                     u32 kmax) {
    u32 *rowcnt = reinterpret_cast<u32 *>(W.flag);
    if (wide)
        maw_row_kernel<true, MODE><<<W.ntiles, FM_MS_NT, 0, ctx->stream>>>(P, rowcnt, W.cnt, W.offs, total, d_left, d_pos, d_len, W.hist, kmax);
    else
        maw_row_kernel<false, MODE><<<W.ntiles, FM_MS_NT, 0, ctx->stream>>>(P, rowcnt, W.cnt, W.offs, total, d_left, d_pos, d_len, W.hist, kmax);
    TC_LAUNCH_CHECK(ctx);
}

// tc_absent_words, tc_absent_words_dev.  maw_left = maw_pos = maw_len = null with capacity 0 is the sizes-only form.
static void absent_words_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 min_len, u32 max_len, u8 *maw_left, u32 *maw_pos,
                               u32 *maw_len, u64 *nmaw, bool dev) {
    if (n > TC_MAX_N || !nmaw) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nmaw;
    *nmaw = 0;
    if (min_len < 2 || (max_len != 0 && max_len < min_len)) TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 2, max_len is 0 or at least min_len");
    const bool sizes_only = !maw_left && !maw_pos && !maw_len && cap == 0;
    if (!sizes_only && (!maw_left || !maw_pos || !maw_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (n == 0) return;
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    const u64 slots = cap < 512 * N ? cap : 512 * N;    // (a row has at most 512 words)
    u8 *d_left = maw_left;
    u32 *d_pos = maw_pos, *d_len = maw_len;
    MawWork W;
    MawArgs P;
    P.min_len = min_len; P.max_len = max_len;
    const bool wide = maw_prepare(ctx, W, text, n, dev, 0, P, [&](Arena &A) {
        if (!dev && !sizes_only) {
            d_left = A.get<u8>(slots + 16);
            d_pos = A.get<u32>(slots + 1);
            d_len = A.get<u32>(slots + 1);
        }
    });
    maw_rows<MAW_COUNT>(ctx, W, P, wide, 0, nullptr, nullptr, nullptr, 0);
    const u64 need = tc_read_total(ctx, W.cnt, W.ntiles, W.tsum, W.offs, cap, sizes_only, nmaw, "word");
    if (!sizes_only && need) {
        maw_rows<MAW_FILL>(ctx, W, P, wide, need, d_left, d_pos, d_len, 0);
        if (!dev) {
            tc_d2h(ctx, maw_left, d_left, need);
            tc_d2h(ctx, maw_pos, d_pos, need * sizeof(u32));
            tc_d2h(ctx, maw_len, d_len, need * sizeof(u32));
        }
    }
    tc_sync_check(ctx);
}

// tc_absent_word_profile (hist in host memory), tc_absent_word_profile_dev (text and hist in HBM)
static void absent_word_profile_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 kmax, u64 *hist, u64 *total, bool dev) {
    if (n > TC_MAX_N || !hist) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (kmax < 2 || kmax > MAW_MAX_KMAX) TC_FAIL(ctx, TC_ERR_ARG, "kmax is 2 .. 4096");
    const size_t bytes = ((size_t)kmax + 1) * sizeof(u64);
    if (total) *total = 0;
    if (n == 0) {
        if (dev) {
            tc_memset_async(ctx, hist, 0, bytes);
            tc_sync_check(ctx);
        } else {
            memset(hist, 0, bytes);
        }
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    MawWork W;
    MawArgs P;
    P.min_len = 2; P.max_len = 0;
    const bool wide = maw_prepare(ctx, W, text, n, dev, kmax, P, [](Arena &) {});
    tc_memset_async(ctx, W.hist, 0, bytes + sizeof(u64));
    maw_rows<MAW_HIST>(ctx, W, P, wide, 0, nullptr, nullptr, nullptr, kmax);
    if (dev) TC_HIP(ctx, hipMemcpyAsync(hist, W.hist, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    else tc_d2h(ctx, hist, W.hist, bytes);
    tc_d2h(ctx, &ctx->h_scalars[9], W.hist + kmax + 1, sizeof(u64));
    tc_sync_check(ctx);
    if (total) *total = ctx->h_scalars[9];
}
