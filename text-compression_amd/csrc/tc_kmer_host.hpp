// tc_kmer_host.hpp -- host side of the k-mer list, spectrum and profile (tc_kmer.hpp has the kernels and the definitions):
// scratch, the launch sequences, and the bodies of tc_kmers / tc_kmers_dev / tc_kmers_esa_dev, tc_kmer_spectrum /
// tc_kmer_spectrum_esa_dev and tc_kmer_profile / tc_kmer_profile_esa_dev.  Included by textcomp.hip after tc_esa_plan.hpp:
// the text forms build their ESA by esa_plan (no last column kept, no tree) and then run the launch sequence of the _esa_dev
// form.
#pragma once
#include "tc_kmer.hpp"

// What one call needs behind the enhanced suffix array: 8 bytes per tile of KM_TILE rows (the tiles' last boundaries and
// their carries), 16 per tile for the counts and first slots of the list plus the scan's tile sums, one word for the
// spectrum's distinct count and 2 (kmax + 1) words for the profile.  Nothing per row.
struct KmWork {
    u32 ntiles = 0;
    u32 *last = nullptr, *carry = nullptr;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    u64 *word = nullptr;    // the spectrum's distinct count
    u64 *prof = nullptr;    // the profile's two histograms
    void carve(Arena &A, u64 N, bool list, u32 kmax) {
        ntiles = (u32)(N / KM_TILE + 1);        // the tiles cover the rows 0 .. N: the virtual row closes the last group
        last = A.get<u32>(ntiles);
        carry = A.get<u32>(ntiles);
        if (list) {
            cnt = A.get<u64>(ntiles);
            offs = A.get<u64>(ntiles + 1);
            tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
        }
        word = A.get<u64>(1);
        if (kmax) prof = A.get<u64>(2 * ((size_t)kmax + 1));
    }
};

static u32 km_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 ? 1u : 0u; }

// carry[t] for every tile: the last boundary of any earlier tile
static void km_carries(tc_ctx *ctx, const KmWork &W, const u32 *d_lcp, u64 N, u32 k) {
    km_tile_kernel<<<W.ntiles, KM_NT, 0, ctx->stream>>>(d_lcp, N, k, km_aligned(d_lcp), W.last);
    TC_LAUNCH_CHECK(ctx);
    km_carry_kernel<<<1, 1024, 0, ctx->stream>>>(W.last, W.carry, W.ntiles);
    TC_LAUNCH_CHECK(ctx);
}

static void km_list_args(tc_ctx *ctx, u32 k, u32 min_occ, u32 max_occ, const u32 *kpos, const u32 *kocc, u64 cap, bool *sizes_only) {
    if (k == 0 || min_occ == 0 || (max_occ != 0 && max_occ < min_occ)) TC_FAIL(ctx, TC_ERR_ARG, "k and min_occ are at least 1, max_occ is 0 or at least min_occ");
    *sizes_only = !kpos && !kocc && cap == 0;
    if (!*sizes_only && (!kpos || !kocc)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
}

// The list from an ESA in HBM: the carries, the count pass, the scan of the tiles' counts, the host reads the total, the
// fill pass.  Returns the count; a capacity that is too small throws after *nk is set.
static u64 km_list_run(tc_ctx *ctx, const KmWork &W, const u32 *d_sa, const u32 *d_lcp, u64 N, u32 k, u32 min_occ, u32 max_occ,
                       u32 *d_pos, u32 *d_occ, u32 *d_row, u64 cap, bool sizes_only, u64 *nk) {
    hipStream_t s = ctx->stream;
    const u32 al = km_aligned(d_lcp);
    km_carries(ctx, W, d_lcp, N, k);
    km_pass_kernel<KM_COUNT><<<W.ntiles, KM_NT, 0, s>>>(d_sa, d_lcp, N, k, min_occ, max_occ, al, W.carry, W.cnt, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, W.cnt, W.ntiles, W.tsum, W.offs, cap, sizes_only, nk, "k-mer");
    if (!sizes_only && need) {
        km_pass_kernel<KM_FILL><<<W.ntiles, KM_NT, 0, s>>>(d_sa, d_lcp, N, k, min_occ, max_occ, al, W.carry, nullptr, W.offs, d_pos, d_occ, d_row, nullptr, 0, nullptr);
        TC_LAUNCH_CHECK(ctx);
    }
    return need;
}

// The spectrum from an ESA in HBM into d_hist (zeroed here); the distinct count is left in W.word.
static void km_spectrum_run(tc_ctx *ctx, const KmWork &W, const u32 *d_sa, const u32 *d_lcp, u64 N, u32 k, u32 bins, u64 *d_hist) {
    tc_memset_async(ctx, d_hist, 0, (size_t)bins * sizeof(u64));
    tc_memset_async(ctx, W.word, 0, sizeof(u64));
    km_carries(ctx, W, d_lcp, N, k);
    km_pass_kernel<KM_HIST><<<W.ntiles, KM_NT, 0, ctx->stream>>>(d_sa, d_lcp, N, k, 1u, 0u, km_aligned(d_lcp), W.carry, nullptr, nullptr, nullptr, nullptr, nullptr, d_hist, bins, W.word);
    TC_LAUNCH_CHECK(ctx);
}

// The profile from an LCP array in HBM: the two histograms, then distinct(k) = max(0, n - k + 1) - #{r : lcp[r] >= k} (a
// suffix sum of the first) and unique(k) = #{r in 1 .. n : max(lcp[r], lcp[r + 1]) < k} - min(k - 1, n) (a prefix sum of the
// second).  Synchronises.
static void km_profile_run(tc_ctx *ctx, const KmWork &W, const u32 *d_lcp, u64 N, u32 kmax, u64 *distinct, u64 *unique) {
    const size_t words = 2 * ((size_t)kmax + 1);
    tc_memset_async(ctx, W.prof, 0, words * sizeof(u64));
    const u32 full = tc_cdiv(N, KM_PF_CHUNK), most = tc_persistent_grid(ctx, 4);
    km_profile_kernel<<<full < most ? full : most, KM_PF_NT, 0, ctx->stream>>>(d_lcp, N, kmax, km_aligned(d_lcp), W.prof);
    TC_LAUNCH_CHECK(ctx);
    std::vector<u64> h(words);
    tc_d2h(ctx, h.data(), W.prof, words * sizeof(u64));
    tc_sync_check(ctx);
    const u64 n = N - 1;
    u64 ge = h[kmax];                               // #{r : lcp[r] >= k}, from k = kmax down
    for (u32 k = kmax; k >= 1; k--) {
        distinct[k - 1] = (n >= k ? n - k + 1 : 0) - ge;
        ge += h[k - 1];
    }
    if (unique) {
        u64 lt = 0;                                 // #{r in 1 .. n : max(lcp[r], lcp[r + 1]) < k}
        for (u32 k = 1; k <= kmax; k++) {
            lt += h[(size_t)kmax + 1 + (k - 1)];
            unique[k - 1] = lt - ((u64)(k - 1) < n ? (u64)(k - 1) : n);
        }
    }
}

// tc_kmers, tc_kmers_dev
static void kmers_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 k, u32 min_occ, u32 max_occ, u32 *sa, u32 *kpos, u32 *kocc,
                        u32 *krow, u64 *nk, bool dev) {
    if (n > TC_MAX_N || !nk) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nk;
    *nk = 0;
    bool sizes_only;
    km_list_args(ctx, k, min_occ, max_occ, kpos, kocc, cap, &sizes_only);
    if (n == 0) {
        esa_empty_sa(ctx, sa, dev);
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    const u64 slots = cap < n ? cap : n;        // (a text of n bytes has at most n k-mers)
    u32 *d_pos = kpos, *d_occ = kocc, *d_row = krow;
    Esa E;
    KmWork W;
    EsaOpts o;
    o.sa = dev ? sa : nullptr;
    esa_plan(ctx, E, text, n, dev,
             [&](Arena &A) {
                 if (!dev && !sizes_only) {
                     d_pos = A.get<u32>(slots + 1);
                     d_occ = A.get<u32>(slots + 1);
                     if (krow) d_row = A.get<u32>(slots + 1);
                 }
             },
             [&](Arena &A) { W.carve(A, N, true, 0); }, o);
    const u64 need = km_list_run(ctx, W, E.d_sa, E.d_lcp, N, k, min_occ, max_occ, d_pos, d_occ, d_row, cap, sizes_only, nk);
    if (!dev && !sizes_only && need) {
        tc_d2h(ctx, kpos, d_pos, need * sizeof(u32));
        tc_d2h(ctx, kocc, d_occ, need * sizeof(u32));
        if (krow) tc_d2h(ctx, krow, d_row, need * sizeof(u32));
    }
    if (!dev && sa) tc_d2h(ctx, sa, E.d_sa, N * sizeof(u32));
    tc_sync_check(ctx);
}

// tc_kmers_esa_dev
static void kmers_esa_entry(tc_ctx *ctx, const u32 *d_sa, const u32 *d_lcp, u64 N, u32 k, u32 min_occ, u32 max_occ, u32 *d_pos,
                            u32 *d_occ, u32 *d_row, u64 *nk) {
    if (!d_sa || !d_lcp || N == 0 || N - 1 > TC_MAX_N || !nk) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nk;
    *nk = 0;
    bool sizes_only;
    km_list_args(ctx, k, min_occ, max_occ, d_pos, d_occ, cap, &sizes_only);
    KmWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { W.carve(A, N, true, 0); });
    km_list_run(ctx, W, d_sa, d_lcp, N, k, min_occ, max_occ, d_pos, d_occ, d_row, cap, sizes_only, nk);
    tc_sync_check(ctx);
}

static void km_spectrum_args(tc_ctx *ctx, u32 k, u32 bins, const u64 *hist, const u64 *distinct, const u64 *total) {
    if (!hist || !distinct || !total) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (k == 0 || bins == 0 || bins > KM_MAX_BINS) TC_FAIL(ctx, TC_ERR_ARG, "k is at least 1, bins 1 .. 65536");
}

// tc_kmer_spectrum
static void kmer_spectrum_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 k, u32 bins, u64 *hist, u64 *distinct, u64 *total) {
    if (n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    km_spectrum_args(ctx, k, bins, hist, distinct, total);
    *distinct = 0;
    *total = n >= k ? n - k + 1 : 0;
    if (n == 0) {
        memset(hist, 0, (size_t)bins * sizeof(u64));
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    u64 *d_hist = nullptr;
    Esa E;
    KmWork W;
    esa_plan(ctx, E, text, n, false, [&](Arena &A) { d_hist = A.get<u64>(bins); }, [&](Arena &A) { W.carve(A, N, false, 0); });
    km_spectrum_run(ctx, W, E.d_sa, E.d_lcp, N, k, bins, d_hist);
    tc_d2h(ctx, hist, d_hist, (size_t)bins * sizeof(u64));
    tc_d2h(ctx, &ctx->h_scalars[9], W.word, sizeof(u64));
    tc_sync_check(ctx);
    *distinct = ctx->h_scalars[9];
}

// tc_kmer_spectrum_esa_dev
static void kmer_spectrum_esa_entry(tc_ctx *ctx, const u32 *d_sa, const u32 *d_lcp, u64 N, u32 k, u32 bins, u64 *d_hist,
                                    u64 *distinct, u64 *total) {
    if (!d_sa || !d_lcp || N == 0 || N - 1 > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    km_spectrum_args(ctx, k, bins, d_hist, distinct, total);
    const u64 n = N - 1;
    *distinct = 0;
    *total = n >= k ? n - k + 1 : 0;
    KmWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { W.carve(A, N, false, 0); });
    km_spectrum_run(ctx, W, d_sa, d_lcp, N, k, bins, d_hist);
    tc_d2h(ctx, &ctx->h_scalars[9], W.word, sizeof(u64));
    tc_sync_check(ctx);
    *distinct = ctx->h_scalars[9];
}

// tc_kmer_profile
static void kmer_profile_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 kmax, u64 *distinct, u64 *unique) {
    if (n > TC_MAX_N || !distinct) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (kmax == 0 || kmax > KM_MAX_KMAX) TC_FAIL(ctx, TC_ERR_ARG, "kmax is 1 .. 4096");
    if (n == 0) {
        memset(distinct, 0, (size_t)kmax * sizeof(u64));
        if (unique) memset(unique, 0, (size_t)kmax * sizeof(u64));
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    Esa E;
    KmWork W;
    esa_plan(ctx, E, text, n, false, [](Arena &) {}, [&](Arena &A) { W.carve(A, N, false, kmax); });
    km_profile_run(ctx, W, E.d_lcp, N, kmax, distinct, unique);
}

// tc_kmer_profile_esa_dev
static void kmer_profile_esa_entry(tc_ctx *ctx, const u32 *d_lcp, u64 N, u32 kmax, u64 *distinct, u64 *unique) {
    if (!d_lcp || N == 0 || N - 1 > TC_MAX_N || !distinct) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (kmax == 0 || kmax > KM_MAX_KMAX) TC_FAIL(ctx, TC_ERR_ARG, "kmax is 1 .. 4096");
    KmWork W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { W.carve(A, N, false, kmax); });
    km_profile_run(ctx, W, d_lcp, N, kmax, distinct, unique);
}
