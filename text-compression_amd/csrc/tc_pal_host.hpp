// tc_pal_host.hpp -- host side of the palindromes / inverted repeats of a text (tc_pal.hpp has the kernels and the
// method): scratch, the launch sequence, and the bodies of tc_palindromes / tc_longest_palindrome and their _dev forms.
// Included by textcomp.hip after tc_esa_plan.hpp, whose lower layer (esa_sort: the sort, then the LCP scratch over its dead
// buffers) it runs over the 2n bytes of the joint text, which a kernel makes first, and tc_tr_host.hpp (tr_isa_kernel).
#pragma once
#include "tc_pal.hpp"

// What one call holds in the workspace.  Ahead of the overlay mark, because the sort must leave it alone: the text (host
// forms), the 256 bytes of sigma, the joint text S, its suffix array, inverse suffix array and LCP array (N = 2n + 1
// entries each), the min tree, and what the host forms return.  Behind the mark, one after another over the same bytes:
// the sort's buffers, the LCP's, and then the packed words (one per centre), the tiles' counts and their scan.  Behind
// the sort that is 1 (S) + 3 x 4 (sa, isa, lcp) + 8 (words) = 21 bytes per byte of S, 42 per text byte, plus the tree
// (4 / (f - 1) per byte of S); the sort's own need behind 13 of those bytes where that is larger.
struct PalWork {
    u8 *d_text = nullptr, *d_sigma = nullptr, *d_S = nullptr;
    u32 *d_sa = nullptr, *isa = nullptr, *lcp = nullptr;
    MinTree tree;
    u32 *lcp_min = nullptr;
    LcpScratch lcp_ws;
    u64 *word = nullptr;        // 2n - 1 entries: len << 32 | mm, 0 for none
    u32 ntiles = 0;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;   // one entry per tile of PAL_TILE centres, and the scan's tile sums
    u64 *red = nullptr;         // the reduction's two words
    // everything the sort leaves alone (the text of the host forms is carved before this)
    void carve_kept(const tc_ctx *ctx, Arena &A, u64 n, bool dry) {
        const u64 N = 2 * n + 1;
        d_sigma = A.get<u8>(256);
        d_S = A.get<u8>(2 * n + 16);
        d_sa = esa_sa_arg(A.get<u32>(N), dry);
        isa = A.get<u32>(N);
        lcp = A.get<u32>(N);
        tree.shape(ctx, (u32)N);
        lcp_min = A.get<u32>(tree.words);
    }
    // what follows the ESA, over its dead buffers
    void carve_words(Arena &A, u64 n) {
        const u64 centres = 2 * n - 1;
        ntiles = tc_cdiv(centres, PAL_TILE);
        word = A.get<u64>(centres);
        cnt = A.get<u64>(ntiles);
        offs = A.get<u64>(ntiles + 1);
        tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
        red = A.get<u64>(2);
    }
};

// what both calls refuse before a buffer is touched; *sigma = comp or, for a null comp, the identity (256 bytes of the
// context's pinned header block, from which the table is uploaded)
static const u8 *pal_check(tc_ctx *ctx, u64 n, const u8 *comp, u32 max_mismatch, u32 min_len) {
    if (min_len == 0) TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 1");
    if (max_mismatch > TC_PAL_MAX_MISMATCH) TC_FAIL(ctx, TC_ERR_ARG, "max_mismatch is at most %u", (unsigned)TC_PAL_MAX_MISMATCH);
    if (n > TC_MAX_N / 2) TC_FAIL(ctx, TC_ERR_ARG, "the text and its mirror image together exceed TC_MAX_N");
    u8 *sigma = reinterpret_cast<u8 *>(ctx->h_hdr);
    for (u32 x = 0; x < 256; x++) sigma[x] = comp ? comp[x] : (u8)x;
    for (u32 x = 0; x < 256; x++)
        if (sigma[sigma[x]] != x) TC_FAIL(ctx, TC_ERR_ARG, "comp is not an involution: comp[comp[%u]] = %u", x, (unsigned)sigma[sigma[x]]);
    return sigma;
}

// The joint text, its ESA, the tree and pal_centre_kernel, n >= 1, on the context's stream: W.word holds every centre's
// word afterwards.  text is the caller's device text (dev) or its host text, which becomes the workspace's first carve;
// outputs(A) carves what the host forms return, ahead of everything that is overlaid.
template <class F>
static void pal_words_device(tc_ctx *ctx, PalWork &W, const u8 *text, u64 n, const u8 *sigma, u32 max_mismatch, u32 min_len,
                             bool dev, F &&outputs) {
    const u64 n2 = 2 * n, N = n2 + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    size_t mark = 0;
    auto kept = [&](Arena &A, bool dry) {
        W.d_text = dev ? const_cast<u8 *>(text) : A.get<u8>(n + 16);
        W.carve_kept(ctx, A, n, dry);
        outputs(A);
        mark = A.off;
    };
    {   // the three overlays behind the mark: the sort, the LCP array, the words
        Arena dry(nullptr);
        kept(dry, true);
        esa_sort(ctx, dry, W.d_S, n2, W.d_sa, W.lcp_ws, true);
        dry.rewind(mark);
        W.carve_words(dry, n);
        tc_ws_reserve(ctx, dry.peak);
    }
    if (!dev) esa_fill_text(ctx, text, n, nullptr, 0, false);
    Arena A(ctx->ws);
    kept(A, false);
    hipStream_t s = ctx->stream;
    tc_h2d(ctx, W.d_sigma, sigma, 256);
    pal_joint_kernel<<<tc_cdiv(n, PAL_NT), PAL_NT, 0, s>>>(W.d_text, (u32)n, W.d_sigma, W.d_S);
    TC_LAUNCH_CHECK(ctx);
    esa_sort(ctx, A, W.d_S, n2, W.d_sa, W.lcp_ws, false);
    lcp_device(ctx, W.lcp_ws, W.d_S, n2, W.d_sa, W.lcp);
    tr_isa_kernel<<<tc_cdiv(N, TR_NT), TR_NT, 0, s>>>(W.d_sa, (u32)N, W.isa, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    A.rewind(mark);
    W.carve_words(A, n);
    W.tree.build(ctx, W.lcp, W.lcp_min);
    pal_centre_kernel<<<tc_cdiv(n2 - 1, FM_MS_NT), FM_MS_NT, 0, s>>>(W.d_S, (u32)n, W.isa, W.lcp, W.lcp_min, W.tree.lf, max_mismatch, min_len,
                                                                    W.word);
    TC_LAUNCH_CHECK(ctx);
}

// tc_palindromes, tc_palindromes_dev.  pal_start = pal_len = pal_mm = null with capacity 0 is the sizes-only form; pal_mm
// alone may be null in any call.
static void palindromes_entry(tc_ctx *ctx, const u8 *text, u64 n, const u8 *comp, u32 max_mismatch, u32 min_len, u32 *pal_start,
                              u32 *pal_len, u32 *pal_mm, u64 *npal, bool dev) {
    if (!npal) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *npal;
    *npal = 0;
    const u8 *sigma = pal_check(ctx, n, comp, max_mismatch, min_len);
    const bool sizes_only = !pal_start && !pal_len && !pal_mm && cap == 0;
    if (!sizes_only && (!pal_start || !pal_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (n == 0) return;
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 centres = 2 * n - 1;
    PalWork W;
    u32 *d_start = pal_start, *d_len = pal_len, *d_mm = pal_mm;
    const u64 slots = cap < centres ? cap : centres;    // (at most one palindrome per centre)
    pal_words_device(ctx, W, text, n, sigma, max_mismatch, min_len, dev, [&](Arena &A) {
        if (dev || sizes_only) return;
        d_start = A.get<u32>(slots + 1);
        d_len = A.get<u32>(slots + 1);
        if (pal_mm) d_mm = A.get<u32>(slots + 1);
    });
    hipStream_t s = ctx->stream;
    pal_count_kernel<<<W.ntiles, PAL_NT, 0, s>>>(W.word, centres, W.cnt);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, W.cnt, W.ntiles, W.tsum, W.offs, cap, sizes_only, npal, "palindrome");
    if (!sizes_only && need) {
        pal_fill_kernel<<<W.ntiles, PAL_NT, 0, s>>>(W.word, centres, W.offs, need, d_start, d_len, d_mm);
        TC_LAUNCH_CHECK(ctx);
        if (!dev) {
            tc_d2h(ctx, pal_start, d_start, need * sizeof(u32));
            tc_d2h(ctx, pal_len, d_len, need * sizeof(u32));
            if (pal_mm) tc_d2h(ctx, pal_mm, d_mm, need * sizeof(u32));
        }
    }
    tc_sync_check(ctx);
}

// tc_longest_palindrome, tc_longest_palindrome_dev: the three results are host words in both forms.  The reduction is
// the one of tc_lcp_summary_dev over the packed words: the largest len, of its centres the smallest; the mismatches are
// then read from that centre's word.
static void longest_palindrome_entry(tc_ctx *ctx, const u8 *text, u64 n, const u8 *comp, u32 max_mismatch, u32 *start, u32 *len,
                                     u32 *mm, bool dev) {
    if (!start || !len || !mm) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u8 *sigma = pal_check(ctx, n, comp, max_mismatch, 1);
    if (n == 0) {
        *start = *len = *mm = 0;
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 centres = 2 * n - 1;
    PalWork W;
    pal_words_device(ctx, W, text, n, sigma, max_mismatch, 1, dev, [](Arena &) {});
    hipStream_t s = ctx->stream;
    tc_memset_async(ctx, W.red, 0, 2 * sizeof(u64));
    const u32 full = tc_cdiv(centres, LCP_NT), most = tc_persistent_grid(ctx, 8);
    pal_longest_kernel<<<full < most ? full : most, LCP_NT, 0, s>>>(W.word, centres, W.red);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[8], W.red, 2 * sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    const u64 key = ctx->h_scalars[8];
    const u32 l = (u32)(key >> 32), c = 0xffffffffu - (u32)key;
    u32 m = 0;
    if (l) {
        tc_d2h(ctx, &ctx->h_scalars[9], W.word + c, sizeof(u64));
        TC_HIP(ctx, hipStreamSynchronize(s));
        m = (u32)ctx->h_scalars[9];
    }
    tc_sync_check(ctx);
    *start = l ? (c + 1u - l) >> 1 : 0;
    *len = l;
    *mm = m;
}
