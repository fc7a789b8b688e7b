// tc_esa_plan.hpp -- what the analyses over the enhanced suffix array (suffix array + LCP array) share on the host: the shape
// and the build of a min tree (MinTree), and the workspace plan of sort, LCP array and the stage's own scratch in two layers
// (esa_sort below, esa_plan above).  Included by tc_fm_host.hpp behind tc_fm_ms.hpp (fm_ms_tree_shape,
// fm_lmin_kernel) and by textcomp.hip right after tc_lcp_host.hpp (lcp_device, LcpScratch).
#pragma once
#include "tc_lcp_host.hpp"

// A min tree over `rows` words at the context's fan-out (fm_ms_tree_shape has the layout): one shape serves every tree of a
// call over that many rows.  The kernels take lf and compute the same shape themselves.
struct MinTree {
    u32 lf = 0, levels = 0, words = 0;
    u32 off[FM_MS_MAXLEV + 1], cnt[FM_MS_MAXLEV + 1];
    void shape(const tc_ctx *ctx, u32 rows) {
        lf = fm_log2(ctx->fm_lcp_fanout ? ctx->fm_lcp_fanout : FM_LCP_FANOUT);
        levels = fm_ms_tree_shape(rows, lf, off, cnt, &words);
    }
    // the tree over src[0 .. rows) into dst[0 .. words): one small kernel per level, each over the one below
    void build(tc_ctx *ctx, const u32 *src, u32 *dst) const {
        for (u32 k = 1; k <= levels; k++) {
            u32 *lev = dst + off[k];
            fm_lmin_kernel<<<tc_cdiv(((u64)cnt[k] + 3) & ~(u64)3, 256), 256, 0, ctx->stream>>>(src, cnt[k - 1], lf, lev, cnt[k]);
            TC_LAUNCH_CHECK(ctx);
            src = lev;
        }
    }
};

// The suffix array a plan hands to sa_build.  A dry run carves without a base, so what it carved is null: any non-null value
// tells sa_build that the array is provided.
static u32 *esa_sa_arg(u32 *carved, bool dry) { return dry ? reinterpret_cast<u32 *>(sizeof(u32)) : carved; }

// The lower layer.  A stands at the overlay mark: the sort of d_text[0 .. n), n >= 1, into d_sa behind the mark, then the LCP
// scratch over the sort's dead buffers (A is left behind it; the caller runs lcp_device and rewinds for what comes next).
// kept_L: where the caller holds a last column it carved ahead of the mark, or null -- then it is carved here and dies with
// the sort.  counts: 256 byte counts, or null.  Returns the primary index (a dry run: 0).
static u64 esa_sort(tc_ctx *ctx, Arena &A, const u8 *d_text, u64 n, u32 *d_sa, LcpScratch &lcp_ws, bool dry, u8 *const *kept_L = nullptr,
                    u32 *counts = nullptr) {
    const size_t mark = A.off;
    u64 primary = 0;
    u8 *d_L = kept_L ? *kept_L : A.get<u8>(n + 1 + 16);
    sa_build(ctx, A, d_text, n, d_sa, d_L, &primary, counts, dry);
    A.rewind(mark);
    lcp_ws.carve(ctx, A, n);
    return primary;
}

// The text of a host form is the workspace's first carve: it is filled between the reserve (which may move the workspace) and
// the run.  text2: a second text right behind the first (dev: both are device memory).
static void esa_fill_text(tc_ctx *ctx, const u8 *text, u64 n, const u8 *text2, u64 n2, bool dev) {
    Arena A0(ctx->ws);
    u8 *x = A0.get<u8>(n + n2 + 16);
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    TC_HIP(ctx, hipMemcpyAsync(x, text, n, kind, ctx->stream));
    if (text2) TC_HIP(ctx, hipMemcpyAsync(x + n, text2, n2, kind, ctx->stream));
}

// The upper layer: the ESA of one text in the context's workspace.  Ahead of the mark, in this order: the text (host forms),
// sa (unless the caller gave its own), lcp, the kept last column, and what pre(A) carves -- all of it outlives the sort.
// Behind the mark, one over the other: the sort's buffers, the LCP scratch, and what post(A) carves.
struct Esa {
    u8 *d_text = nullptr, *d_L = nullptr;   // d_L: with keep_L only
    u32 *d_sa = nullptr, *d_lcp = nullptr;
    u64 primary = 0;
    LcpScratch lcp_ws;
};
struct EsaOpts {
    u32 *sa = nullptr;          // the caller's device array for sa (n + 1 entries)
    bool keep_L = false;        // the last column outlives the sort
    u32 *counts = nullptr;      // the sort's 256 byte counts
    const u8 *text2 = nullptr;  // the text is text . text2, n2 bytes more, copied into the first carve in both forms
    u64 n2 = 0;
};
// text: n1 bytes, n1 + n2 >= 1.  Sets ctx->stats, reserves the workspace once, and leaves lcp_device queued on the context's stream.
template <class Pre, class Post>
static void esa_plan(tc_ctx *ctx, Esa &E, const u8 *text, u64 n1, bool dev, Pre &&pre, Post &&post, const EsaOpts &o = EsaOpts()) {
    const u64 n = n1 + o.n2, N = n + 1;
    const bool carve_text = !dev || o.text2;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    auto plan = [&](Arena &A, bool dry) {
        E.d_text = carve_text ? A.get<u8>(n + 16) : const_cast<u8 *>(text);
        E.d_sa = esa_sa_arg(o.sa ? o.sa : A.get<u32>(N), dry);
        E.d_lcp = A.get<u32>(N);
        if (o.keep_L) E.d_L = A.get<u8>(N + 16);
        pre(A);
        const size_t mark = A.off;
        E.primary = esa_sort(ctx, A, E.d_text, n, E.d_sa, E.lcp_ws, dry, o.keep_L ? &E.d_L : nullptr, o.counts);
        A.rewind(mark);
        post(A);
    };
    Arena dry(nullptr);
    plan(dry, true);
    tc_ws_reserve(ctx, dry.peak);
    if (carve_text) esa_fill_text(ctx, text, n1, o.text2, o.n2, dev);
    Arena A(ctx->ws);
    plan(A, false);
    lcp_device(ctx, E.lcp_ws, E.d_text, n, E.d_sa, E.d_lcp);
}

// tc_lcp_array: upload, sort, LCP, download (here and not in tc_lcp_host.hpp, which this file is included after)
static void lcp_array_host_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 *sa, u32 *lcp) {
    if (n > TC_MAX_N || !lcp) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) {
        if (sa) sa[0] = 0;
        lcp[0] = 0;
        return;
    }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 N = n + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    u8 *d_text = nullptr;
    u32 *d_sa = nullptr, *d_lcp = nullptr;
    LcpScratch W;
    // (the lower layer alone: the dry run hands sa_build the null it carved, not esa_sa_arg's value, so it sizes a suffix
    // array of the sort's own as well -- 4 N bytes that the run does not use, reserved since this call exists)
    auto plan = [&](Arena &A, bool dry) {
        d_text = A.get<u8>(n + 16);
        d_sa = A.get<u32>(N);
        d_lcp = A.get<u32>(N);
        esa_sort(ctx, A, d_text, n, d_sa, W, dry);
    };
    Arena dry(nullptr);
    plan(dry, true);
    tc_ws_reserve(ctx, dry.peak);
    esa_fill_text(ctx, text, n, nullptr, 0, false);
    Arena A(ctx->ws);
    plan(A, false);
    lcp_device(ctx, W, d_text, n, d_sa, d_lcp);
    if (sa) tc_d2h(ctx, sa, d_sa, N * sizeof(u32));
    tc_d2h(ctx, lcp, d_lcp, N * sizeof(u32));
    tc_sync_check(ctx);
}

// n = 0 of a call that hands back sa: one row, 0, as tc_suffix_array
static void esa_empty_sa(tc_ctx *ctx, u32 *sa, bool dev) {
    if (sa && dev) {
        tc_memset_async(ctx, sa, 0, sizeof(u32));
        tc_sync_check(ctx);
    } else if (sa) {
        sa[0] = 0;
    }
}
