// tc_lz_host.hpp -- host side of the LPF array, the LZ77 parse and its inverse (tc_lz.hpp has the kernels and the
// algorithm): scratch, the launch sequences, and the bodies of tc_lpf_array / tc_lz_parse / tc_lz_unparse and their _dev
// forms.  Included by textcomp.hip after tc_esa_plan.hpp (esa_plan, MinTree).
#pragma once
#include "tc_lz.hpp"

// the tile of this context's parses: LZ_TILE unless the debug interface set another (tc_dbg_lz_set_tile)
static u32 lz_tile(const tc_ctx *ctx) { return ctx->lz_tile ? ctx->lz_tile : LZ_TILE; }

// What one LPF / parse call holds in the workspace: the ESA of esa_plan (tc_esa_plan.hpp) with what the host forms return
// ahead of the mark, and -- over the sort's and then the LCP's dead buffers -- the two min trees, the packed (lpf, src) array
// and the parse's tables.
struct LzWork : Esa {
    MinTree tree;
    u32 *sa_min = nullptr, *lcp_min = nullptr;
    u64 *pack = nullptr;    // n entries: src << 32 | lpf
    u32 ltile = 0, ntiles = 0;
    u32 *exitp = nullptr;   // n entries (the parse only, like the four below)
    u32 *entry = nullptr;   // one word per tile
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;
    void carve(const tc_ctx *ctx, Arena &A, u64 n, bool parse) {
        tree.shape(ctx, (u32)(n + 1));
        sa_min = A.get<u32>(tree.words);
        lcp_min = A.get<u32>(tree.words);
        pack = A.get<u64>(n);
        if (!parse) return;
        ltile = fm_log2(lz_tile(ctx));
        ntiles = tc_cdiv(n, (u64)1 << ltile);
        exitp = A.get<u32>(n);
        entry = A.get<u32>(ntiles);
        cnt = A.get<u64>(ntiles);
        offs = A.get<u64>(ntiles + 1);
        tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
    }
};

// The ESA, the two trees and lz_lpf_kernel, n >= 1, on the context's stream: W.pack holds (lpf, src) of every position
// afterwards.  text is the caller's device text (dev) or its host text; outputs(A) carves what the host forms return.
template <class F>
static void lz_lpf_device(tc_ctx *ctx, LzWork &W, const u8 *text, u64 n, bool dev, bool parse, F &&outputs) {
    esa_plan(ctx, W, text, n, dev, outputs, [&](Arena &A) { W.carve(ctx, A, n, parse); });
    W.tree.build(ctx, W.d_sa, W.sa_min);
    W.tree.build(ctx, W.d_lcp, W.lcp_min);
    lz_lpf_kernel<<<tc_cdiv(n, 256), 256, 0, ctx->stream>>>(W.d_sa, W.d_lcp, W.sa_min, W.lcp_min, (u32)(n + 1), W.tree.lf, W.pack);
    TC_LAUNCH_CHECK(ctx);
}

template <int MODE>
static void lz_tile_launch(tc_ctx *ctx, const LzWork &W, u64 n, u32 *d_ph_src, u32 *d_ph_len) {
    const size_t lds = (size_t)9 << W.ltile;
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(lz_tile_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    lz_tile_kernel<MODE><<<W.ntiles, LZ_NT, lds, ctx->stream>>>(W.pack, (u32)n, W.ltile, W.exitp, W.entry, W.cnt, W.offs, W.d_text,
                                                               d_ph_src, d_ph_len);
    TC_LAUNCH_CHECK(ctx);
}

// steps a to c of the parse and the scan of the tiles' counts: returns the number of phrases (tc_read_total: the host waits
// for it, *nph is set, a capacity that is too small throws)
static u64 lz_phrase_starts(tc_ctx *ctx, const LzWork &W, u64 n, u64 cap, bool sizes_only, u64 *nph) {
    lz_tile_launch<0>(ctx, W, n, nullptr, nullptr);
    tc_memset_async(ctx, W.entry, 0xff, (size_t)W.ntiles * sizeof(u32));
    lz_chain_kernel<<<1, 64, 0, ctx->stream>>>(W.exitp, (u32)n, W.ltile, W.entry);
    TC_LAUNCH_CHECK(ctx);
    lz_tile_launch<1>(ctx, W, n, nullptr, nullptr);
    return tc_read_total(ctx, W.cnt, W.ntiles, W.tsum, W.offs, cap, sizes_only, nph, "phrase");
}

// tc_lpf_array, tc_lpf_array_dev
static void lpf_array_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 *lpf, u32 *src, bool dev) {
    if (n > TC_MAX_N || !lpf) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) return;
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    LzWork W;
    u32 *d_lpf = lpf, *d_src = src;
    lz_lpf_device(ctx, W, text, n, dev, false, [&](Arena &A) {
        if (dev) return;
        d_lpf = A.get<u32>(n);
        if (src) d_src = A.get<u32>(n);
    });
    lz_unpack_kernel<<<tc_cdiv(n, 256), 256, 0, ctx->stream>>>(W.pack, (u32)n, d_lpf, d_src);
    TC_LAUNCH_CHECK(ctx);
    if (!dev) {
        tc_d2h(ctx, lpf, d_lpf, n * sizeof(u32));
        if (src) tc_d2h(ctx, src, d_src, n * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// tc_lz_parse, tc_lz_parse_dev.  ph_src = ph_len = null with capacity 0 is the sizes-only form: the count, TC_OK.
static void lz_parse_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 *ph_src, u32 *ph_len, u64 *nph, bool dev) {
    if (n > TC_MAX_N || !nph) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nph;
    *nph = 0;
    const bool sizes_only = !ph_src && !ph_len && cap == 0;
    if (!sizes_only && (!ph_src || !ph_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (n == 0) return;
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    LzWork W;
    u32 *d_ph_src = ph_src, *d_ph_len = ph_len;
    const u64 slots = cap < n ? cap : n;        // (a text of n bytes has at most n phrases)
    lz_lpf_device(ctx, W, text, n, dev, true, [&](Arena &A) {
        if (dev || sizes_only) return;
        d_ph_src = A.get<u32>(slots + 1);
        d_ph_len = A.get<u32>(slots + 1);
    });
    const u64 need = lz_phrase_starts(ctx, W, n, cap, sizes_only, nph);
    if (!sizes_only) {
        lz_tile_launch<2>(ctx, W, n, d_ph_src, d_ph_len);
        if (!dev) {
            tc_d2h(ctx, ph_src, d_ph_src, need * sizeof(u32));
            tc_d2h(ctx, ph_len, d_ph_len, need * sizeof(u32));
        }
    }
    tc_sync_check(ctx);
}

// tc_lz_unparse, tc_lz_unparse_dev.  text = null with capacity 0 is the sizes-only form.  A bad phrase list is TC_ERR_ARG
// before anything is written to text, as is a total above cap (TC_ERR_CAPACITY).
static void lz_unparse_entry(tc_ctx *ctx, const u32 *ph_src, const u32 *ph_len, u64 nph, u8 *text, u64 *nbytes, bool dev) {
    if (!nbytes) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nbytes;
    *nbytes = 0;
    if (!text && cap) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (nph == 0) return;
    if (!ph_src || !ph_len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    // (every phrase is at least one byte: more phrases than TC_MAX_N make a text above it)
    if (nph > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "unparse: a bad phrase list (%llu phrases make more than TC_MAX_N bytes)", (unsigned long long)nph);
    u32 *u_src = nullptr, *u_len = nullptr;             // the host form's copies of the phrase list
    u64 *d_len64 = nullptr, *d_starts = nullptr, *d_tsum = nullptr;
    u32 *d_flags = nullptr, *d_par[2] = {nullptr, nullptr};
    u8 *d_out = text;
    const u32 *d_src = ph_src, *d_len = ph_len;
    hipStream_t s = ctx->stream;
    // The phrases' starts, their total and the verdict on the list, with room for `room` output bytes behind them.  It runs
    // twice: the byte total sizes the parent arrays, and a reserve may move the workspace, so the second run carves and
    // computes everything again (a scan over the phrases: small next to the rounds over the bytes).
    auto starts_of = [&](u64 room) {
        tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
            if (!dev) {
                u_src = A.get<u32>(nph);
                u_len = A.get<u32>(nph);
                if (room) d_out = A.get<u8>(room + 16);
            }
            d_len64 = A.get<u64>(nph);
            d_starts = A.get<u64>(nph + 1);
            d_tsum = A.get<u64>(tc_cdiv(nph, SCAN_TILE) + 2);
            d_flags = A.get<u32>(2);                    // [0] a bad list, [1] a round changed something
            if (room) {
                d_par[0] = A.get<u32>(room);
                d_par[1] = A.get<u32>(room);
            }
        });
        if (!dev) {
            tc_h2d(ctx, u_src, ph_src, nph * sizeof(u32));
            tc_h2d(ctx, u_len, ph_len, nph * sizeof(u32));
            d_src = u_src;
            d_len = u_len;
        }
        const u32 pgrid = tc_cdiv(nph, 256);
        tc_memset_async(ctx, d_flags, 0, 2 * sizeof(u32));
        lz_un_len_kernel<<<pgrid, 256, 0, s>>>(d_len, nph, d_len64);
        TC_LAUNCH_CHECK(ctx);
        const u64 *d_total = tc_scan64(ctx, d_len64, nph, d_tsum, d_starts);
        lz_un_check_kernel<<<pgrid, 256, 0, s>>>(d_src, d_len, d_starts, nph, d_flags);
        TC_LAUNCH_CHECK(ctx);
        tc_d2h(ctx, &ctx->h_scalars[9], d_total, sizeof(u64));
        tc_d2h(ctx, &ctx->h_scalars[10], d_flags, sizeof(u32));
        TC_HIP(ctx, hipStreamSynchronize(s));
    };
    starts_of(0);
    const u64 need = ctx->h_scalars[9];
    if ((u32)ctx->h_scalars[10] || need > TC_MAX_N)
        TC_FAIL(ctx, TC_ERR_ARG, "unparse: a bad phrase list (a copy's source lies before its own start; a literal has len 0 and src <= 255; at most TC_MAX_N bytes in all)");
    *nbytes = need;
    if (need > cap) {
        if (!text) return;                              // sizes only
        TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu bytes, have %llu", (unsigned long long)need, (unsigned long long)cap);
    }
    starts_of(need);
    if ((u32)ctx->h_scalars[10] || ctx->h_scalars[9] != need)      // (a device list another stream changed between the two runs)
        TC_FAIL(ctx, TC_ERR_ARG, "unparse: the phrase list changed during the call");
    const u32 total = (u32)need, grid = tc_cdiv(need, 256);
    lz_un_parent_kernel<<<grid, 256, 0, s>>>(d_src, d_len, d_starts, nph, total, d_par[0], d_out);
    TC_LAUNCH_CHECK(ctx);
    // parent = parent o parent; whether a round still moved anything is looked at every fourth round
    const int most = ceil_log2_u64(need) + 1;
    int cur = 0;
    for (int done = 0; done < most;) {
        tc_memset_async(ctx, d_flags + 1, 0, sizeof(u32));
        for (int k = 0; k < 4 && done < most; k++, done++) {
            lz_un_jump_kernel<<<grid, 256, 0, s>>>(d_par[cur], d_par[cur ^ 1], total, d_flags + 1);
            TC_LAUNCH_CHECK(ctx);
            cur ^= 1;
        }
        tc_d2h(ctx, &ctx->h_scalars[10], d_flags + 1, sizeof(u32));
        TC_HIP(ctx, hipStreamSynchronize(s));
        if (!(u32)ctx->h_scalars[10]) break;
    }
    lz_un_gather_kernel<<<grid, 256, 0, s>>>(d_par[cur], total, d_out);
    TC_LAUNCH_CHECK(ctx);
    if (!dev) tc_d2h(ctx, text, d_out, need);
    tc_sync_check(ctx);
}
