// tc_sus_host.hpp -- host side of the unique substrings (tc_sus.hpp has the kernels and the method): scratch, the launch
// sequence, and the bodies of tc_unique_prefixes, tc_unique_substrings, tc_shortest_unique and their _dev forms.  Included by
// textcomp.hip after tc_esa_plan.hpp: the ESA is esa_plan's, with nothing kept but sa and lcp.
#pragma once
#include "tc_sus.hpp"

// What one call holds in the workspace: the text (host form), sa and lcp (4 + 4 bytes per text byte) and what a host form
// returns ahead of the overlay mark; behind it, over the sort's and then the LCP's dead buffers, what the call is after:
//   prefixes  up (4; the caller's array in the _dev form): 12 bytes per text byte
//   list      up (4), and 16 bytes per tile of SUS_TILE positions: 12 bytes per text byte; the list's 8 bytes per MUS lie ahead of
//             the mark in the host form
//   point     up (4), mlen (4), endof / pred (4), nxt (4), the min tree (4 / (f - 1)) and 8 bytes per tile: 24 bytes per text
//             byte, 32 with the host form's two arrays
// -- the sort's own need behind the first 8 where that is larger.
enum { SUS_PREFIX = 0, SUS_LIST = 1, SUS_POINT = 2 };
struct SusWork : Esa {
    u32 *up = nullptr;
    u32 ntiles = 0;
    u64 *cnt = nullptr, *offs = nullptr, *tsum = nullptr;       // the list
    MinTree tree;                                               // the point call: the tree is over the n entries of mlen
    u32 *mlen = nullptr, *mlen_min = nullptr, *pred = nullptr, *nxt = nullptr, *tmax = nullptr, *tmin = nullptr;
    void carve(const tc_ctx *ctx, Arena &A, u64 n, int what, u32 *up_dev) {
        up = up_dev ? up_dev : A.get<u32>(n + 1);
        ntiles = tc_cdiv(n, SUS_TILE);
        if (what == SUS_LIST) {
            cnt = A.get<u64>(ntiles);
            offs = A.get<u64>(ntiles + 1);
            tsum = A.get<u64>(tc_cdiv(ntiles, SCAN_TILE) + 2);
        } else if (what == SUS_POINT) {
            tree.shape(ctx, (u32)n);
            mlen = A.get<u32>(n + 4);       // (level 0 of the tree is read 16 bytes at a time)
            mlen_min = A.get<u32>(tree.words);
            pred = A.get<u32>(n);
            nxt = A.get<u32>(n + 1);
            tmax = A.get<u32>(ntiles);
            tmin = A.get<u32>(ntiles);
        }
    }
};

// The ESA of the text (n >= 1) and up, on the context's stream.  outputs(A) carves what a host form returns, ahead of
// everything that is overlaid; up_dev: the caller's array of tc_unique_prefixes_dev.
template <class F>
static void sus_prepare(tc_ctx *ctx, SusWork &W, const u8 *text, u64 n, bool dev, int what, u32 *up_dev, F &&outputs) {
    const u64 N = n + 1;
    esa_plan(ctx, W, text, n, dev, outputs, [&](Arena &A) { W.carve(ctx, A, n, what, up_dev); });
    sus_prefix_kernel<<<tc_cdiv(N, FM_MS_NT), FM_MS_NT, 0, ctx->stream>>>(W.d_sa, W.d_lcp, (u32)N, W.up);
    TC_LAUNCH_CHECK(ctx);
}

// tc_unique_prefixes (up in host memory), tc_unique_prefixes_dev (text and up in HBM)
static void unique_prefixes_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 *up, bool dev) {
    if (n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) return;
    if (!text || !up) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    SusWork W;
    sus_prepare(ctx, W, text, n, dev, SUS_PREFIX, dev ? up : nullptr, [](Arena &) {});
    if (!dev) tc_d2h(ctx, up, W.up, n * sizeof(u32));
    tc_sync_check(ctx);
}

// tc_unique_substrings, tc_unique_substrings_dev.  mus_start = mus_len = null with capacity 0 is the sizes-only form.
static void unique_substrings_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 min_len, u32 max_len, u32 *mus_start, u32 *mus_len,
                                    u64 *nmus, bool dev) {
    if (n > TC_MAX_N || !nmus) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nmus;
    *nmus = 0;
    if (min_len == 0 || (max_len != 0 && max_len < min_len))
        TC_FAIL(ctx, TC_ERR_ARG, "min_len is at least 1; max_len is 0 (no limit) or at least min_len");
    const bool sizes_only = !mus_start && !mus_len && cap == 0;
    if (!sizes_only && (!mus_start || !mus_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (n == 0) return;
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 slots = cap < n ? cap : n;        // (a text of n bytes has at most n MUS)
    u32 *d_start = mus_start, *d_len = mus_len;
    SusWork W;
    sus_prepare(ctx, W, text, n, dev, SUS_LIST, nullptr, [&](Arena &A) {
        if (!dev && !sizes_only) {
            d_start = A.get<u32>(slots + 1);
            d_len = A.get<u32>(slots + 1);
        }
    });
    hipStream_t s = ctx->stream;
    sus_mark_kernel<SUS_COUNT><<<W.ntiles, SUS_NT, 0, s>>>(W.up, (u32)n, min_len, max_len, nullptr, nullptr, W.cnt, nullptr, 0, nullptr, nullptr);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = tc_read_total(ctx, W.cnt, W.ntiles, W.tsum, W.offs, cap, sizes_only, nmus, "MUS");
    if (!sizes_only && need) {
        sus_mark_kernel<SUS_FILL><<<W.ntiles, SUS_NT, 0, s>>>(W.up, (u32)n, min_len, max_len, nullptr, nullptr, nullptr, W.offs, need, d_start, d_len);
        TC_LAUNCH_CHECK(ctx);
        if (!dev) {
            tc_d2h(ctx, mus_start, d_start, need * sizeof(u32));
            tc_d2h(ctx, mus_len, d_len, need * sizeof(u32));
        }
    }
    tc_sync_check(ctx);
}

// tc_shortest_unique, tc_shortest_unique_dev.  sus_start may be null.
static void shortest_unique_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 *sus_start, u32 *sus_len, bool dev) {
    if (n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) return;
    if (!text || !sus_len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u32 *d_start = sus_start, *d_len = sus_len;
    SusWork W;
    sus_prepare(ctx, W, text, n, dev, SUS_POINT, nullptr, [&](Arena &A) {
        if (!dev) {
            if (sus_start) d_start = A.get<u32>(n);
            d_len = A.get<u32>(n);
        }
    });
    hipStream_t s = ctx->stream;
    tc_memset_async(ctx, W.pred, 0, n * sizeof(u32));
    sus_mark_kernel<SUS_MARK><<<W.ntiles, SUS_NT, 0, s>>>(W.up, (u32)n, 1, 0, W.mlen, W.pred, nullptr, nullptr, 0, nullptr, nullptr);
    TC_LAUNCH_CHECK(ctx);
    sus_reduce_kernel<<<W.ntiles, SUS_NT, 0, s>>>(W.pred, W.mlen, (u32)n, W.tmax, W.tmin);
    TC_LAUNCH_CHECK(ctx);
    sus_spine_kernel<<<1, 1024, 0, s>>>(W.tmax, W.tmin, W.ntiles, (u32)n);
    TC_LAUNCH_CHECK(ctx);
    sus_scan_kernel<<<W.ntiles, SUS_NT, 0, s>>>(W.pred, W.mlen, (u32)n, W.tmax, W.tmin, W.nxt);
    TC_LAUNCH_CHECK(ctx);
    W.tree.build(ctx, W.mlen, W.mlen_min);
    sus_point_kernel<<<tc_cdiv(n, FM_MS_NT), FM_MS_NT, 0, s>>>(W.mlen, W.mlen_min, W.pred, W.nxt, (u32)n, W.tree.lf, d_start, d_len);
    TC_LAUNCH_CHECK(ctx);
    if (!dev) {
        if (sus_start) tc_d2h(ctx, sus_start, d_start, n * sizeof(u32));
        tc_d2h(ctx, sus_len, d_len, n * sizeof(u32));
    }
    tc_sync_check(ctx);
}
