// tc_decode_host.hpp -- the host side of the decode path: it drives the inverse BWT (ibwt_device and its phases; the
// kernels and the scheme they implement are in tc_ibwt.hpp), the inverse MTF (kernels: tc_mtf.hpp), the inverse RLE
// (kernels: tc_rle.hpp) and the fused decode of a block, decode_device.
#pragma once
#include <type_traits>
#include <algorithm>
#include "tc_encode_host.hpp"
#include "tc_ibwt.hpp"

// ---- inverse BWT ---------------------------------------------------------------
// What one inverse BWT of N symbols carves, whichever way it goes.
struct IbwtBuffers {
    u32 K, Kx, Kt;   // splitters: one per IBWT_S rows + slots for walks that outgrow a record (ibwt_walk1_kernel)
    u32 *d_counts, *v0, *v1, *hist, *nx[2], *ds[2], *seglen, *ovlist, *lf_bcnt;
    u64 *k0, *k1, *rstatus;
    u8 *segflag;
    uint4 *lf_lines;
    // k0 holds the segment records ((K + Kx) * IBWT_SEGCAP ~ 16.5 N bytes; in the scatter path it is not used for keys at all)
    u8 *seg() const { return reinterpret_cast<u8 *>(k0); }
    void carve(Arena &A, u64 N) {
        K = tc_cdiv(N, IBWT_S);
        d_counts = A.get<u32>(260);
        // (k0 doubles as the segment record buffer after the sort: K * IBWT_SEGCAP bytes)
        Kx = K / 32 + 256, Kt = K + Kx;
        k0 = A.get<u64>(N > (u64)Kt * (IBWT_SEGCAP / 8) ? N : (u64)Kt * (IBWT_SEGCAP / 8));
        k1 = A.get<u64>(N);
        v0 = A.get<u32>(N);
        v1 = A.get<u32>(N);
        hist = A.get<u32>(RDX_MAX_PASSES * RDX_BINS);
        rstatus = A.get<u64>(radix_status_words(N));
        for (int i = 0; i < 2; i++) nx[i] = A.get<u32>(Kt + 1);
        for (int i = 0; i < 2; i++) ds[i] = A.get<u32>(Kt + 1);
        seglen = A.get<u32>(Kt + 1);
        segflag = A.get<u8>(Kt + 1);
        ovlist = A.get<u32>(Kt + 1);
        lf_lines = A.get<uint4>(((size_t)(N / LF_ROWS) + 1) * 4);   // LF walk: N / 2 bytes
        lf_bcnt = A.get<u32>(((size_t)tc_cdiv(N, LF_BLOCK) + 1) * 4);
    }
};

// The two step functions of a walk, each with its two launches: walk1 records every splitter's segment (nx[0] / ds[0],
// counters ctr[0] = overflowed records, ctr[1] = extra slots taken), walk2 writes the nov listed segments that did not
// fit their record at their final offsets (nxf / dsf: the ranked chain).
struct IbwtPosWalker {
    const u32 *spos;
    CTable ct;
    void walk1(tc_ctx *ctx, const IbwtBuffers &B, u32 N, u32 rewalk, u32 *ctr, u32 xcap, u32 segcap) const {
        ibwt_walk1_kernel<<<tc_cdiv(B.K, 256), 256, 0, ctx->stream>>>(spos, N, B.K, B.nx[0], B.ds[0], ct, B.seg(), B.seglen,
                                                                     B.segflag, rewalk, ctr, B.ovlist, ctr + 1, xcap, segcap);
    }
    void walk2(tc_ctx *ctx, const IbwtBuffers &B, u32 N, const u32 *nxf, const u32 *dsf, u32 nov, u8 *d_text) const {
        ibwt_walk2_kernel<<<tc_cdiv(nov, 256), 256, 0, ctx->stream>>>(spos, N, B.K, nxf, dsf, ctx->d_scalars, ct, d_text,
                                                                     B.ovlist, nov, ctx->d_err);
    }
};
struct IbwtLfWalker {
    const uint4 *lines;
    const u32 *prim;
    LfTable tb;
    void walk1(tc_ctx *ctx, const IbwtBuffers &B, u32 N, u32 rewalk, u32 *ctr, u32 xcap, u32 segcap) const {
        ibwt_lfwalk1_kernel<<<tc_cdiv(B.K, 256), 256, 0, ctx->stream>>>(lines, N, B.K, prim, tb, B.nx[0], B.ds[0], B.seg(),
                                                                       B.seglen, B.segflag, rewalk, ctr, B.ovlist, ctr + 1,
                                                                       xcap, segcap);
    }
    void walk2(tc_ctx *ctx, const IbwtBuffers &B, u32 N, const u32 *nxf, const u32 *dsf, u32 nov, u8 *d_text) const {
        ibwt_lfwalk2_kernel<<<tc_cdiv(nov, 256), 256, 0, ctx->stream>>>(lines, N, B.K, prim, tb, nxf, dsf, ctx->d_scalars,
                                                                       d_text, B.ovlist, nov);
    }
};

// Ranks the chain of the first Ka slots from nx[0] / ds[0]: splitter 0 made the terminal, pointer jumping, the length of
// row e's cycle to d_scalars[6].  Returns which of the two nx / ds buffers holds the result.
static int ibwt_rank_chain(tc_ctx *ctx, const IbwtBuffers &B, u32 Ka) {
    hipStream_t s = ctx->stream;
    ibwt_terminal_kernel<<<1, 1, 0, s>>>(B.nx[0], B.ds[0], ctx->d_scalars);
    TC_LAUNCH_CHECK(ctx);
    int cur = 0;
    for (int r = 0; r < ceil_log2_u64(Ka) + 1; r++) {
        ibwt_jump_kernel<<<tc_cdiv(Ka, 256), 256, 0, s>>>(B.nx[cur], B.ds[cur], B.nx[cur ^ 1], B.ds[cur ^ 1], Ka);
        TC_LAUNCH_CHECK(ctx);
        cur ^= 1;
    }
    ibwt_len_kernel<<<1, 1, 0, s>>>(B.nx[cur], B.ds[cur], ctx->d_scalars, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    return cur;
}

// walks (recording) -> chain ranking -> copy-out, shared by both step functions.  First with slots for
// walks that outgrow their record; if those run out (or TC_IBWT_REWALK asks for the old way) once more
// without, the long segments then being walked a second time.  What the attempts did stays in the context
// (tc_dbg_ibwt_walk).
template <class Walker>
static void ibwt_walk_rank_copy(tc_ctx *ctx, const IbwtBuffers &B, u64 N, const Walker &walker, bool reversed,
                                u8 *d_text, u64 *n_out) {
    hipStream_t s = ctx->stream;
    const u32 rewalk = (u32)env_int("TC_IBWT_REWALK", 0);
    // (tests: records "full" after fewer symbols, so that small inputs reach the extra slots and their exhaustion)
    u32 segcap = (u32)env_int("TC_IBWT_SEGCAP", IBWT_SEGCAP) & ~15u;
    if (segcap < 16 || segcap > IBWT_SEGCAP) segcap = IBWT_SEGCAP;
    u32 *nov_ctr = reinterpret_cast<u32 *>(ctx->d_scalars + 17);   // [0] overflowed records, [1] extra slots taken
    for (int attempt = rewalk ? 1 : 0; attempt < 2; attempt++) {
        const u32 xcap = attempt == 0 ? B.Kx : 0u;
        const u32 Ka = B.K + xcap;    // slots that take part in the ranking
        tc_memset_async(ctx, ctx->d_scalars + 17, 0, sizeof(u64));
        if (xcap) {
            ibwt_extra_init_kernel<<<tc_cdiv(xcap, 256), 256, 0, s>>>(B.K, Ka, B.nx[0], B.ds[0], B.seglen, B.segflag);
            TC_LAUNCH_CHECK(ctx);
        }
        walker.walk1(ctx, B, (u32)N, rewalk, nov_ctr, xcap, segcap);
        TC_LAUNCH_CHECK(ctx);
        const int cur = ibwt_rank_chain(ctx, B, Ka);
        tc_d2h(ctx, &ctx->h_scalars[6], ctx->d_scalars + 6, sizeof(u64));
        tc_d2h(ctx, &ctx->h_scalars[17], ctx->d_scalars + 17, sizeof(u64));
        TC_HIP(ctx, hipStreamSynchronize(s));
        const u32 nov = (u32)(ctx->h_scalars[17] & 0xffffffffu), taken = (u32)(ctx->h_scalars[17] >> 32);
        ctx->ibwt_attempts++;
        ctx->ibwt_overflowed = nov;
        ctx->ibwt_extra_taken = taken;
        if (xcap && taken > xcap) continue;   // slots ran out: the old way
        if (reversed)
            ibwt_copy_rev_kernel<<<tc_cdiv(Ka, 4), 256, 0, s>>>(Ka, B.nx[cur], B.ds[cur], ctx->d_scalars, B.seg(), B.seglen,
                                                               B.segflag, d_text);
        else
            ibwt_copy_kernel<<<tc_cdiv(Ka, 4), 256, 0, s>>>(Ka, B.nx[cur], B.ds[cur], ctx->d_scalars, B.seg(), B.seglen,
                                                           B.segflag, d_text, ctx->d_err);
        TC_LAUNCH_CHECK(ctx);
        if (nov) {
            walker.walk2(ctx, B, (u32)N, B.nx[cur], B.ds[cur], nov, d_text);
            TC_LAUNCH_CHECK(ctx);
        }
        TC_HIP(ctx, hipStreamSynchronize(s));
        break;
    }
    const u64 Lc = ctx->h_scalars[6];
    *n_out = Lc ? Lc - 1 : 0;
}

// small alphabet, one Nothing: walk by LF over the packed last column (tc_ibwt.hpp).  syms = the
// byte values in order (codes 0..nsym-1); cnt = their occurrences, or null: counted on the
// device (then the walk is only taken if the column holds exactly one Nothing and nothing else
// than these symbols -- returns false otherwise, nothing written)
template <class Acc>
static bool ibwt_lf_walk(tc_ctx *ctx, const IbwtBuffers &B, Acc acc, u64 N, const u8 *syms, u32 nsym, const u32 *cnt,
                         u8 *d_text, u64 *n_out) {
    hipStream_t s = ctx->stream;
    Lut8 l8;
    u32 *prim = reinterpret_cast<u32 *>(ctx->d_scalars + 24);   // 4 words + 4 totals
    IbwtLfWalker w = {B.lf_lines, prim, {}};
    for (int v = 0; v < 257; v++) l8.v[v] = 0xff;
    l8.v[0] = 0;
    for (u32 c = 0; c < nsym; c++) {
        // (a CodeAcc stream already holds the codes: its "symbol" c is code c)
        l8.v[(std::is_same<Acc, CodeAcc>::value ? c : (u32)syms[c]) + 1] = (u8)c;
        w.tb.sym[c] = syms[c];
    }
    const u32 nb = tc_cdiv(N, LF_BLOCK);
    tc_memset_async(ctx, prim, 0, 4 * sizeof(u64));
    tc_memset_async(ctx, prim, 0xff, sizeof(u32));
    lf_count_kernel<Acc><<<nb, 256, 0, s>>>(acc, (u32)N, l8, B.lf_bcnt, prim);
    TC_LAUNCH_CHECK(ctx);
    lf_scan_kernel<<<1, 1024, 0, s>>>(B.lf_bcnt, nb, prim + 4);
    TC_LAUNCH_CHECK(ctx);
    u32 tot[5] = {0, 0, 0, 0, 0};
    if (cnt) {
        for (u32 c = 0; c < nsym; c++) tot[c] = cnt[c];
    } else {
        tc_d2h(ctx, &ctx->h_scalars[24], ctx->d_scalars + 24, 4 * sizeof(u64));
        TC_HIP(ctx, hipStreamSynchronize(s));
        const u32 *hp = reinterpret_cast<const u32 *>(&ctx->h_scalars[24]);
        if (hp[1] != 1 || hp[2] != 0) return false;
        u64 sum4 = 0;
        for (int c = 0; c < 4; c++) { tot[c] = hp[4 + c]; sum4 += hp[4 + c]; }
        tot[0] -= 1;                       // the Nothing was counted as code 0
        tot[4] = (u32)(N - sum4);
    }
    u32 crow = 1;   // row 0 is the Nothing's
    for (u32 c = 0; c < 5; c++) {
        w.tb.C[c] = crow;
        crow += tot[c];
    }
    lf_build_kernel<Acc><<<nb, 256, 0, s>>>(acc, (u32)N, l8, B.lf_bcnt, B.lf_lines);
    TC_LAUNCH_CHECK(ctx);
    ibwt_walk_rank_copy(ctx, B, N, w, /*reversed=*/true, d_text, n_out);
    return true;
}

// 1. sorted (symbol, position): the positions by symbol (Nothing first), *ct = the first sorted row of every code
template <class Acc>
static const u32 *ibwt_sorted_positions(tc_ctx *ctx, const IbwtBuffers &B, Acc acc, u64 N, const u32 *counts257,
                                        const Alphabet &al, CTable *ct) {
    hipStream_t s = ctx->stream;
    Lut16 lut;
    u32 acc_c = 0;
    for (int v = 0; v < 257; v++) lut.v[v] = al.code_of_sym[v];
    for (u32 c = 0; c < al.sigma; c++) {
        ct->c[c] = acc_c;
        ct->sym[c] = al.sym_of_code[c];
        acc_c += counts257[al.sym_of_code[c] + 1];
    }
    ct->c[al.sigma] = (u32)N;
    ct->sigma = al.sigma;
    if (al.sigma <= 256 && env_int("TC_IBWT_SCATTER", 1) != 0) {
        for (u32 c = al.sigma; c < 260; c++) ct->c[c] = (u32)N;   // codes that do not occur
        const u32 stiles = tc_cdiv(N, ISC_TILE);
        u32 *sticket = reinterpret_cast<u32 *>(B.rstatus + (size_t)stiles * 256);
        tc_memset_async(ctx, B.rstatus, 0, ((size_t)stiles * 256 + 2) * sizeof(u64));
        ibwt_scatter_kernel<Acc><<<stiles, ISC_NT, 0, s>>>(acc, (u32)N, lut, *ct, B.v0, B.rstatus, sticket, ctx->d_err);
        TC_LAUNCH_CHECK(ctx);
        return B.v0;
    }
    ibwt_keys_kernel<Acc><<<tc_cdiv(N, 256), 256, 0, s>>>(acc, (u32)N, lut, B.k0);
    TC_LAUNCH_CHECK(ctx);
    RadixPlan plan;
    plan.add_range(0, ceil_log2_u64(al.sigma) > 0 ? ceil_log2_u64(al.sigma) : 1);
    RadixBuffers rb;
    rb.keys = B.k0; rb.keys_alt = B.k1; rb.vals = B.v0; rb.vals_alt = B.v1;
    rb.hist = B.hist; rb.status = B.rstatus;
    radix_sort_pairs(ctx, rb, (u32)N, plan, /*gen_idx=*/true, /*hist_ready=*/false);
    return rb.vals;
}

// Inverse BWT of an accessor stream; d_text receives *n_out bytes (<= N).
// alphabet (optional, fused decode): the sorted symbols the stream can hold (the block's MTF list);
// lets the small-alphabet path count on the device instead of taking a histogram first
template <class Acc>
static void ibwt_device(tc_ctx *ctx, Arena &A, Acc acc, u64 N, const u32 *counts257, u8 *d_text,
                        u64 *n_out, bool dry, const i16 *alphabet = nullptr, u32 nalphabet = 0) {
    IbwtBuffers B;
    B.carve(A, N);
    if (dry) return;
    *n_out = 0;
    ctx->ibwt_attempts = ctx->ibwt_overflowed = ctx->ibwt_extra_taken = 0;
    const bool lf_on = N > 1 && env_int("TC_IBWT_LF", 1) != 0;
    if (lf_on && !counts257 && alphabet && nalphabet >= 2 && nalphabet <= 6 && alphabet[0] == -1) {
        // the caller knows the alphabet: no histogram pass
        u8 syms[5];
        bool ok = true;
        for (u32 i = 1; i < nalphabet; i++) {
            ok = ok && alphabet[i] > alphabet[i - 1] && alphabet[i] <= 255;
            syms[i - 1] = (u8)alphabet[i];
        }
        if (ok && ibwt_lf_walk(ctx, B, acc, N, syms, nalphabet - 1, nullptr, d_text, n_out)) return;
    }
    if constexpr (std::is_same<Acc, CodeAcc>::value) {
        *n_out = ~0ull;   // a code stream only takes the LF walk; the caller falls back to symbols
    } else {
        u32 local[257];
        if (!counts257) {
            sym_hist_host<Acc>(ctx, acc, N, B.d_counts, local);
            counts257 = local;
        }
        if (counts257[0] == 0) return;  // no Nothing: magicInverseBWT returns empty (:173-174)
        Alphabet al;
        al.build(counts257);
        if (lf_on && counts257[0] == 1 && al.sigma <= 6) {
            u8 syms[5];
            u32 cnt[5];
            for (u32 c = 1; c < al.sigma; c++) {
                syms[c - 1] = (u8)al.sym_of_code[c];
                cnt[c - 1] = counts257[al.sym_of_code[c] + 1];
            }
            if (ibwt_lf_walk(ctx, B, acc, N, syms, al.sigma - 1, cnt, d_text, n_out)) return;
        }
        IbwtPosWalker w;
        w.spos = ibwt_sorted_positions(ctx, B, acc, N, counts257, al, &w.ct);
        // 2. splitter walks (recording the symbols passed), chain ranking, copy-out
        ibwt_walk_rank_copy(ctx, B, N, w, /*reversed=*/false, d_text, n_out);
    }
}

// ---- inverse MTF ---------------------------------------------------------------
template <int ROWS>
static void imtf_launch(tc_ctx *ctx, const u16 *d_idx, u64 N, u32 sigma, u16 *perms, u32 chunks,
                        const SymTab &tab, i16 *d_out) {
    hipStream_t s = ctx->stream;
    imtf_summary_kernel<ROWS><<<chunks, 64, 0, s>>>(d_idx, N, sigma, perms, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    imtf_scan_kernel<ROWS><<<1, 64 * MTFG_SCAN_WAVES, 0, s>>>(perms, chunks);
    TC_LAUNCH_CHECK(ctx);
    imtf_apply_kernel<ROWS><<<chunks, 64, 0, s>>>(d_idx, N, sigma, perms, tab, d_out);
    TC_LAUNCH_CHECK(ctx);
}

// sigma <= 256: one chunk per lane (tc_mtf.hpp, "inverse MTF, lane chunks")
template <int ROWS>
static void imtf_lane_launch(tc_ctx *ctx, const u16 *d_idx, u64 N, u32 sigma, u16 *perms,
                             const SymTab &tab, i16 *d_out) {
    hipStream_t s = ctx->stream;
    GmiArgs a;
    a.N = N; a.sigma = sigma; a.ls = ((sigma + 3) / 4) | 1u;
    a.idx = d_idx; a.perms = perms; a.tab = tab; a.out = d_out; a.err = ctx->d_err;
    const u32 tiles = tc_cdiv(N, GM_TILE);
    const size_t lds = gm_lds_bytes(a.ls);
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(imtf_gm_kernel<ROWS, false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(imtf_gm_kernel<ROWS, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    imtf_gm_kernel<ROWS, false><<<tiles, GM_NT, lds, s>>>(a);
    TC_LAUNCH_CHECK(ctx);
    imtf_scan_kernel<ROWS><<<1, 64 * MTFG_SCAN_WAVES, 0, s>>>(perms, tiles);
    TC_LAUNCH_CHECK(ctx);
    imtf_gm_kernel<ROWS, true><<<tiles, GM_NT, lds, s>>>(a);
    TC_LAUNCH_CHECK(ctx);
}

// seqFromMTF: initial list = sort(unique(list)) (MTF/Internal.hs:214).
// list = 16 nibbles in a register (tc_mtf.hpp, "inverse MTF, sigma <= 16"); t_perm: tiles + 1 words
template <class IT, class OT>
static void imtf_nib_device(tc_ctx *ctx, u64 *t_perm, const IT *d_idx, u64 N, u32 sigma, const SymTab &tab,
                            OT *d_out) {
    hipStream_t s = ctx->stream;
    const u32 tiles = tc_cdiv(N, MTF_TILE);
    imtf_nib_summary_kernel<IT><<<tiles, MTF_NT, 0, s>>>(d_idx, N, sigma, t_perm, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    imtf_nib_scan_kernel<<<1, MTF_NT, 0, s>>>(t_perm, tiles);
    TC_LAUNCH_CHECK(ctx);
    imtf_nib_apply_kernel<IT, OT><<<tiles, MTF_NT, 0, s>>>(d_idx, N, sigma, t_perm, tab, d_out, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
}

// primary / d_idx_rw (fused decode only): the row of the one sentinel and the same index buffer,
// writable -- lets sigma = 257 take the 256-symbol lane chunks (tc_mtf.hpp, "sigma = 257")
static void mtf_decode_device(tc_ctx *ctx, Arena &A, const u16 *d_idx, u64 N, const i16 *list,
                              u32 nlist, i16 *d_out, bool dry, i64 primary = -1, u16 *d_idx_rw = nullptr) {
    const u32 chunks = tc_cdiv(N, MTFG_CH);
    u16 *perms = A.get<u16>(((size_t)chunks + 1) * 320);
    const u32 tiles257 = tc_cdiv(N, M257_TILE);
    u16 *tmax = A.get<u16>((size_t)tiles257 + 8);
    u32 *fix = A.get<u32>(512);
    if (dry) return;
    bool seen[257] = {false};
    for (u32 i = 0; i < nlist; i++) {
        if (list[i] < -1 || list[i] > 255) TC_FAIL(ctx, TC_ERR_ARG, "list symbol out of range");
        seen[list[i] + 1] = true;
    }
    SymTab tab;
    u32 sigma = 0;
    for (int v = 0; v < 257; v++)
        if (seen[v]) tab.v[sigma++] = (i16)(v - 1);
    for (u32 v = sigma; v < 260; v++) tab.v[v] = 0;
    if (sigma == 257 && d_idx_rw && primary > 0 && (u64)primary < N && env_int("TC_MTF_WAVE_CHUNKS", 0) == 0 &&
        env_int("TC_MTF_SENTINEL_SPLIT", 1) != 0) {
        hipStream_t s = ctx->stream;
        u64 *res = ctx->d_scalars + 20;
        tc_memset_async(ctx, res, 0, 3 * sizeof(u64));
        imtf257_tmax_kernel<<<tiles257, 256, 0, s>>>(d_idx, N, tmax);
        TC_LAUNCH_CHECK(ctx);
        imtf257_chain_kernel<<<1, 256, 0, s>>>(d_idx, N, (u64)primary, tmax, fix, res);
        TC_LAUNCH_CHECK(ctx);
        u32 grid = tc_cdiv(N, 256 * 16);
        if (grid > 8192) grid = 8192;
        imtf257_check_kernel<<<grid, 256, 0, s>>>(d_idx, N, (u64)primary, fix, res);
        TC_LAUNCH_CHECK(ctx);
        tc_d2h(ctx, &ctx->h_scalars[20], res, 3 * sizeof(u64));
        TC_HIP(ctx, hipStreamSynchronize(s));
        if (ctx->h_scalars[22] == 0) {
            imtf257_apply_kernel<<<1, 512, 0, s>>>(d_idx_rw, (u64)primary, fix, res);
            TC_LAUNCH_CHECK(ctx);
            SymTab bytes;
            for (int v = 0; v < 260; v++) bytes.v[v] = (i16)(v < 256 ? v : 0);
            imtf_lane_launch<4>(ctx, d_idx, N, 256, perms, bytes, d_out);
            imtf257_sentinel_kernel<<<1, 1, 0, s>>>(d_out, (u64)primary);
            TC_LAUNCH_CHECK(ctx);
            return;
        }
        // not the index stream of a BWT with its sentinel at `primary`: the nine-bit path below
    }
    if (sigma <= 16 && env_int("TC_MTF_FORCE_GENERAL", 0) == 0 && env_int("TC_MTF_WAVE_CHUNKS", 0) == 0) {
        imtf_nib_device<u16, i16>(ctx, reinterpret_cast<u64 *>(perms), d_idx, N, sigma, tab, d_out);
        return;
    }
    if (sigma <= 256 && env_int("TC_MTF_WAVE_CHUNKS", 0) == 0) {
        const u32 rows = (sigma + 63) / 64;
        if (rows <= 1) imtf_lane_launch<1>(ctx, d_idx, N, sigma, perms, tab, d_out);
        else if (rows == 2) imtf_lane_launch<2>(ctx, d_idx, N, sigma, perms, tab, d_out);
        else if (rows == 3) imtf_lane_launch<3>(ctx, d_idx, N, sigma, perms, tab, d_out);
        else imtf_lane_launch<4>(ctx, d_idx, N, sigma, perms, tab, d_out);
    } else if (sigma <= 64) imtf_launch<1>(ctx, d_idx, N, sigma, perms, chunks, tab, d_out);
    else if (sigma <= 128) imtf_launch<2>(ctx, d_idx, N, sigma, perms, chunks, tab, d_out);
    else imtf_launch<5>(ctx, d_idx, N, sigma, perms, chunks, tab, d_out);
}

// ---- inverse RLE ---------------------------------------------------------------
template <class SymT, class OutT = SymT>
static void rle_decode_device(tc_ctx *ctx, Arena &A, const u32 *d_counts, const SymT *d_syms,
                              u64 nruns, bool has_nothing, OutT *d_out, u64 cap, u64 *N_out,
                              bool dry) {
    const u32 ntiles = tc_cdiv(nruns, RLD_TILE);
    u64 *status = A.get<u64>((size_t)ntiles + 4);
    const u32 huge_cap = (u32)(cap / RLE_HUGE + 2);
    HugeRun *huge = A.get<HugeRun>(huge_cap);
    u32 *nhuge = A.get<u32>(4);
    if (dry) return;
    hipStream_t s = ctx->stream;
    tc_memset_async(ctx, nhuge, 0, 4 * sizeof(u32));
    tc_memset_async(ctx, status, 0, ((size_t)ntiles + 4) * sizeof(u64));
    tc_memset_async(ctx, ctx->d_scalars + 7, 0, sizeof(u64));
    RleDecArgs a;
    a.counts = d_counts; a.syms = d_syms; a.nruns = nruns; a.has_nothing = has_nothing ? 1 : 0;
    a.cap = cap; a.out = d_out; a.status = status;
    a.ticket = reinterpret_cast<u32 *>(status + ntiles + 2);
    a.total = ctx->d_scalars + 7; a.err = ctx->d_err;
    a.huge = huge; a.nhuge = nhuge; a.huge_cap = huge_cap; a.ntiles = ntiles;
    u32 grid = tc_persistent_grid_for(ctx, rle_decode_fused_kernel<SymT, OutT>, RLD_NT, 8);
    if (grid > ntiles) grid = ntiles;
    rle_decode_fused_kernel<SymT, OutT><<<grid, RLD_NT, 0, s>>>(a);
    TC_LAUNCH_CHECK(ctx);
    rle_fill_huge_kernel<OutT><<<tc_persistent_grid(ctx, 4), 256, 0, s>>>(huge, nhuge, huge_cap, cap, d_out);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[7], ctx->d_scalars + 7, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    *N_out = ctx->h_scalars[7];   // > cap: the caller reports TC_ERR_CAPACITY (nothing past cap was written)
}

// ---- fused decode: runs -> MTF indices -> BWT symbols -> text -------------------
static void decode_device(tc_ctx *ctx, const tc_block *blk, u8 *d_text) {
    const u64 n = blk->n, N = n + 1;
    u16 *d_idx = nullptr;
    i16 *d_sym = nullptr;
    u64 got = 0, n_out = 0;
    i16 sorted_list[TC_MAX_SIGMA];
    {
        const u32 sg = blk->sigma <= TC_MAX_SIGMA ? blk->sigma : 0;
        for (u32 i = 0; i < sg; i++) sorted_list[i] = blk->final_list[i];
        std::sort(sorted_list, sorted_list + sg);
    }
    // small alphabets (a proper list: distinct symbols in range): the byte-wide pipeline
    bool small = blk->sigma >= 1 && blk->sigma <= 16 && env_int("TC_MTF_FORCE_GENERAL", 0) == 0 &&
                 env_int("TC_MTF_WAVE_CHUNKS", 0) == 0 && env_int("TC_DECODE_BYTES", 1) != 0;
    for (u32 i = 0; small && i < blk->sigma; i++)
        small = sorted_list[i] >= -1 && sorted_list[i] <= 255 && (i == 0 || sorted_list[i] > sorted_list[i - 1]);
    const bool small_lf = small && blk->sigma >= 2 && blk->sigma <= 6 && sorted_list[0] == -1 && N > 1 &&
                          env_int("TC_IBWT_LF", 1) != 0;
    auto plan = [&](Arena &A, bool dry) {
        d_idx = A.get<u16>(N + 64);
        d_sym = A.get<i16>(N + 64);
        const size_t mark = A.off;   // every stage below carves from here: its scratch overlays the one before
        if (small) {
            // sigma <= 16: indices and codes one byte each all the way (half the traffic of the u16 / i16 forms)
            u8 *d_idx8 = reinterpret_cast<u8 *>(d_idx);
            u8 *d_code8 = reinterpret_cast<u8 *>(d_idx) + ((N + 64 + 15) & ~(u64)15);   // second half of d_idx
            rle_decode_device<u16, u8>(ctx, A, blk->run_count, blk->run_value, blk->nruns, false, d_idx8, N, &got, dry);
            if (!dry && got != N)
                TC_FAIL(ctx, TC_ERR_MALFORMED, "runs expand to %llu symbols, block says %llu",
                        (unsigned long long)got, (unsigned long long)N);
            A.rewind(mark);
            u64 *t_perm = A.get<u64>((size_t)tc_cdiv(N, MTF_TILE) + 2);
            SymTab tab;
            for (u32 v = 0; v < 260; v++) tab.v[v] = v < blk->sigma ? sorted_list[v] : (i16)0;
            bool walked = false;
            if (small_lf) {
                if (!dry) imtf_nib_device<u8, u8>(ctx, t_perm, d_idx8, N, blk->sigma, tab, d_code8);
                A.rewind(mark);
                CodeAcc cacc{d_code8};
                ibwt_device<CodeAcc>(ctx, A, cacc, N, nullptr, d_text, &n_out, dry, sorted_list, blk->sigma);
                walked = dry || n_out != ~0ull;
                if (!walked) {   // not one Nothing / a code outside the list: the symbol path decides
                    u32 g = tc_cdiv(N, 256 * 8);
                    codes_to_syms_kernel<<<g > 8192 ? 8192 : g, 256, 0, ctx->stream>>>(d_code8, N, tab, d_sym);
                    TC_LAUNCH_CHECK(ctx);
                }
            } else if (!dry) {
                imtf_nib_device<u8, i16>(ctx, t_perm, d_idx8, N, blk->sigma, tab, d_sym);
            }
            A.rewind(mark);
            if (!walked || dry) {
                SymAcc sacc{d_sym};
                u64 n2 = 0;
                ibwt_device<SymAcc>(ctx, A, sacc, N, nullptr, d_text, &n2, dry);
                if (!walked) n_out = n2;
            }
            return;
        }
        rle_decode_device<u16>(ctx, A, blk->run_count, blk->run_value, blk->nruns, false, d_idx, N,
                               &got, dry);
        if (!dry && got != N)
            TC_FAIL(ctx, TC_ERR_MALFORMED, "runs expand to %llu symbols, block says %llu",
                    (unsigned long long)got, (unsigned long long)N);
        A.rewind(mark);
        mtf_decode_device(ctx, A, d_idx, N, blk->final_list, blk->sigma, d_sym, dry, (i64)blk->primary, d_idx);
        A.rewind(mark);
        SymAcc acc{d_sym};
        // the symbols the stream can hold: the block's MTF list, sorted
        ibwt_device<SymAcc>(ctx, A, acc, N, nullptr, d_text, &n_out, dry, sorted_list, blk->sigma);
    };
    tc_ws_plan(ctx, 0, plan);
    tc_sync_check(ctx);
    if (n_out != n)
        TC_FAIL(ctx, TC_ERR_MALFORMED, "block decodes to %llu bytes, header says %llu",
                (unsigned long long)n_out, (unsigned long long)n);
}
