// tc_encode_host.hpp -- host orchestration of the encode path (device pointers in,
// device pointers out): MTF, RLE and the encode entry; the suffix sort's driver is tc_sa_host.hpp,
// included below.  Included by textcomp.hip only.
#pragma once
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "tc_mtf.hpp"
#include "tc_radix_host.hpp"
#include "tc_rle.hpp"
#include "tc_pack.hpp"
#include "tc_sa.hpp"
#include "tc_msd.hpp"
#include "tc_seg.hpp"
#include "tc_chain.hpp"

// ---------------------------------------------------------------- small helpers
static inline void tc_memset_async(tc_ctx *ctx, void *p, int v, size_t bytes) {
    TC_HIP(ctx, hipMemsetAsync(p, v, bytes, ctx->stream));
}
static inline void tc_d2h(tc_ctx *ctx, void *dst, const void *src, size_t bytes) {
    TC_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
}
static inline void tc_h2d(tc_ctx *ctx, void *dst, const void *src, size_t bytes) {
    TC_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
}
static inline int ceil_log2_u64(u64 v) {  // bits needed to hold values < v
    int b = 0;
    while (b < 63 && (1ull << b) < v) b++;
    return b;
}
static inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

// Alphabet of a Seq (Maybe Word8): counts257[0] = #Nothing, [1+b] = #byte b.
// nubSeq' (reference MTF/Internal.hs:79-99): present symbols, sorted, Nothing first.
struct Alphabet {
    u32 sigma = 0;
    i16 sym_of_code[TC_MAX_SIGMA];
    u16 code_of_sym[TC_MAX_SIGMA];  // index = sym + 1
    void build(const u32 *counts257) {
        sigma = 0;
        for (int v = 0; v < 257; v++) {
            code_of_sym[v] = 0;
            if (counts257[v]) {
                code_of_sym[v] = (u16)sigma;
                sym_of_code[sigma++] = (i16)(v - 1);
            }
        }
    }
};

// ------------------------------------------------------------------ suffix array
#include "tc_sa_host.hpp"

// ------------------------------------------------------------------- accessors
template <class Acc>
static Acc make_acc(const void *d_src, i64 primary);
template <>
BwtAcc make_acc<BwtAcc>(const void *d_src, i64 primary) {
    return BwtAcc{reinterpret_cast<const u8 *>(d_src), primary};
}
template <>
SymAcc make_acc<SymAcc>(const void *d_src, i64) {
    return SymAcc{reinterpret_cast<const i16 *>(d_src)};
}
template <>
U16Acc make_acc<U16Acc>(const void *d_src, i64) {
    return U16Acc{reinterpret_cast<const u16 *>(d_src)};
}

// Symbol histogram of an accessor stream -> host counts257.
template <class Acc>
static void sym_hist_host(tc_ctx *ctx, Acc acc, u64 N, u32 *d_counts, u32 *counts257) {
    tc_memset_async(ctx, d_counts, 0, 260 * sizeof(u32));
    u32 grid = tc_cdiv(N, 256 * 32);
    if (grid > 2048) grid = 2048;
    sym_hist_kernel<Acc><<<grid, 256, 0, ctx->stream>>>(acc, N, d_counts);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, counts257, d_counts, 257 * sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
}

// ------------------------------------------------------------------------- MTF
template <class Acc, int ROWS>
static void mtf_general_launch(tc_ctx *ctx, Acc acc, u64 N, const Lut16 &lut, u16 *lists,
                               u32 *seen, u32 chunks, u16 *d_idx) {
    hipStream_t s = ctx->stream;
    mtf_gen_summary_kernel<Acc, ROWS><<<chunks, 64, 0, s>>>(acc, N, lut, lists, seen);
    TC_LAUNCH_CHECK(ctx);
    mtf_gen_scan_kernel<ROWS><<<1, 64 * MTFG_SCAN_WAVES, 0, s>>>(lists, seen, chunks);
    TC_LAUNCH_CHECK(ctx);
    mtf_gen_apply_kernel<Acc, ROWS><<<chunks, 64, 0, s>>>(acc, N, lut, lists, d_idx);
    TC_LAUNCH_CHECK(ctx);
}

// any sigma > 16: timestamps (tc_mtf.hpp, "general path, timestamps"); the final list lands in `flist`
template <class Acc, int ROWS>
static void mtf_ts_launch(tc_ctx *ctx, Acc acc, u64 N, const Lut16 &lut, u32 sigma, u32 *ts, u32 *seg, u16 *flist,
                          u16 *d_idx) {
    hipStream_t s = ctx->stream;
    const u32 chunks = tc_cdiv(N, TS_CH), nseg = tc_cdiv(chunks, TS_SEG);
    mtf_ts_last_kernel<Acc><<<chunks, 256, 0, s>>>(acc, N, lut, ts);
    TC_LAUNCH_CHECK(ctx);
    mtf_ts_scan_kernel<0><<<nseg, TS_STRIDE, 0, s>>>(ts, chunks, seg, nseg, sigma);
    TC_LAUNCH_CHECK(ctx);
    mtf_ts_scan_kernel<1><<<1, TS_STRIDE, 0, s>>>(ts, chunks, seg, nseg, sigma);
    TC_LAUNCH_CHECK(ctx);
    mtf_ts_scan_kernel<2><<<nseg, TS_STRIDE, 0, s>>>(ts, chunks, seg, nseg, sigma);
    TC_LAUNCH_CHECK(ctx);
    mtf_ts_final_kernel<<<1, TS_STRIDE, 0, s>>>(seg + (size_t)nseg * TS_STRIDE, sigma, flist);
    TC_LAUNCH_CHECK(ctx);
    mtf_ts_apply_kernel<Acc, ROWS><<<tc_cdiv(chunks, TS_WPB * TS_ILP), 64 * TS_WPB, 0, s>>>(acc, N, lut, ts, d_idx, chunks);
    TC_LAUNCH_CHECK(ctx);
}

// sigma <= 256: one chunk per lane (tc_mtf.hpp, "general path, lane chunks")
template <class Acc, int ROWS>
static void mtf_lane_launch(tc_ctx *ctx, Acc acc, u64 N, const Alphabet &al, u16 *lists, u32 *seen,
                            u16 *d_idx) {
    hipStream_t s = ctx->stream;
    GmArgs a;
    a.N = N; a.sigma = al.sigma; a.ls = ((al.sigma + 3) / 4) | 1u;
    for (int v = 0; v < 257; v++) a.lut.v[v] = (u8)al.code_of_sym[v];
    a.lists = lists; a.seen = seen; a.idx = d_idx;
    const u32 tiles = tc_cdiv(N, GM_TILE);
    const size_t lds = gm_lds_bytes(a.ls);
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(mtf_gm_kernel<Acc, ROWS, false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(mtf_gm_kernel<Acc, ROWS, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    mtf_gm_kernel<Acc, ROWS, false><<<tiles, GM_NT, lds, s>>>(acc, a);
    TC_LAUNCH_CHECK(ctx);
    mtf_gen_scan_kernel<ROWS><<<1, 64 * MTFG_SCAN_WAVES, 0, s>>>(lists, seen, tiles);
    TC_LAUNCH_CHECK(ctx);
    mtf_gm_kernel<Acc, ROWS, true><<<tiles, GM_NT, lds, s>>>(acc, a);
    TC_LAUNCH_CHECK(ctx);
}

// seqToMTF on the device.  counts257 (host) may be null: then it is measured here.
// d_idx8 (optional): for sigma <= 16 the indices are written THERE, one byte each (*used8 = true)
template <class Acc>
static void mtf_encode_device(tc_ctx *ctx, Arena &A, Acc acc, u64 N, const u32 *counts257,
                              u16 *d_idx, i16 *final_list, u32 *sigma, bool dry, u8 *d_idx8 = nullptr,
                              bool *used8 = nullptr) {
    const u32 tiles = tc_cdiv(N, MTF_TILE);
    const u32 chunks = tc_cdiv(N, MTFG_CH);
    u32 *d_counts = A.get<u32>(260);
    u64 *t_perm = A.get<u64>(tiles + 1);
    u32 *t_mask = A.get<u32>(tiles + 1 > 512 ? tiles + 1 : 512);
    u16 *lists = A.get<u16>(((size_t)chunks + 4) * 320);   // (also: [N / TS_CH + 1][TS_STRIDE] u32 timestamps)
    u32 *seen = A.get<u32>(chunks + 1);
    u32 *ts_seg = A.get<u32>(((size_t)tc_cdiv(tc_cdiv(N, TS_CH), TS_SEG) + 2) * TS_STRIDE);
    u16 *ts_flist = A.get<u16>(TS_STRIDE);
    if (dry) return;
    hipStream_t s = ctx->stream;
    u32 local[257];
    if (!counts257) {
        sym_hist_host<Acc>(ctx, acc, N, d_counts, local);
        counts257 = local;
    }
    Alphabet al;
    al.build(counts257);
    *sigma = al.sigma;
    const bool force_general = env_int("TC_MTF_FORCE_GENERAL", 0) != 0;
    if (al.sigma <= 16 && !force_general) {
        Lut8 lut;
        for (int v = 0; v < 257; v++) lut.v[v] = (u8)al.code_of_sym[v];
        // fast path: every tile recovers its incoming list by a short backward scan
        bool fast_ok = false;
        const bool scan_failed = ctx->mtf_fastin_failed != 0;   // (this record's one-kernel attempt: long runs in the column)
        ctx->mtf_fastin_failed = 0;
        if (env_int("TC_MTF_FASTIN", 1) != 0 && !scan_failed) {
            u32 *flag = reinterpret_cast<u32 *>(ctx->d_scalars + 15);
            tc_memset_async(ctx, flag, 0, sizeof(u64));
            if (d_idx8 && al.sigma <= 8 && env_int("TC_MTF_SMALL", 1) != 0)   // (a DNA record: the list in 32 bits)
                mtf_nib_apply_kernel<Acc, true, u8, true><<<tiles, MTF_NT, 0, s>>>(acc, N, lut, t_perm, d_idx8, al.sigma, flag);
            else if (d_idx8) mtf_nib_apply_kernel<Acc, true, u8><<<tiles, MTF_NT, 0, s>>>(acc, N, lut, t_perm, d_idx8, al.sigma, flag);
            else mtf_nib_apply_kernel<Acc, true><<<tiles, MTF_NT, 0, s>>>(acc, N, lut, t_perm, d_idx, al.sigma, flag);
            TC_LAUNCH_CHECK(ctx);
            mtf_nib_final_kernel<Acc><<<1, 64, 0, s>>>(acc, N, lut, al.sigma, t_perm + tiles, flag);
            TC_LAUNCH_CHECK(ctx);
            tc_d2h(ctx, &ctx->h_scalars[15], ctx->d_scalars + 15, sizeof(u64));
            tc_d2h(ctx, &ctx->h_scalars[8], t_perm + tiles, sizeof(u64));
            TC_HIP(ctx, hipStreamSynchronize(s));
            fast_ok = ((u32)ctx->h_scalars[15]) == 0;
        }
        if (!fast_ok) {
            mtf_nib_summary_kernel<Acc><<<tiles, MTF_NT, 0, s>>>(acc, N, lut, t_perm, t_mask);
            TC_LAUNCH_CHECK(ctx);
            mtf_nib_scan_kernel<<<1, MTF_NT, 0, s>>>(t_perm, t_mask, tiles);
            TC_LAUNCH_CHECK(ctx);
            if (d_idx8) mtf_nib_apply_kernel<Acc, false, u8><<<tiles, MTF_NT, 0, s>>>(acc, N, lut, t_perm, d_idx8, al.sigma, nullptr);
            else mtf_nib_apply_kernel<Acc, false><<<tiles, MTF_NT, 0, s>>>(acc, N, lut, t_perm, d_idx, al.sigma, nullptr);
            TC_LAUNCH_CHECK(ctx);
            tc_d2h(ctx, &ctx->h_scalars[8], t_perm + tiles, sizeof(u64));
            TC_HIP(ctx, hipStreamSynchronize(s));
        }
        u64 perm = ctx->h_scalars[8];
        for (u32 i = 0; i < al.sigma; i++) final_list[i] = al.sym_of_code[(perm >> (4 * i)) & 15];
        if (used8) *used8 = d_idx8 != nullptr;
    } else {
        Lut16 lut;
        for (int v = 0; v < 257; v++) lut.v[v] = al.code_of_sym[v];
        int rows;
        u32 last;  // slot of the final list
        // timestamps: the default beyond 64 symbols (1 GiB: uniform bytes 258 -> 37 ms, ASCII 81 -> 26 ms,
        // Zipf words over all byte values 126 -> ~40 ms; up to 64 symbols the lane chunks are ahead on
        // BWT-like streams: Zipf text, sigma 28, 12 against 23 ms).  TC_MTF_TS=0: never, 2: whenever sigma > 16.
        const int ts_mode = env_int("TC_MTF_TS", 1);
        if (ts_mode != 0 && (al.sigma > 64 || ts_mode == 2) && N + 300 < (1ull << 32)) {
            rows = (int)((al.sigma + 63) / 64);
            u32 *ts = reinterpret_cast<u32 *>(lists);
            if (rows == 1) mtf_ts_launch<Acc, 1>(ctx, acc, N, lut, al.sigma, ts, ts_seg, ts_flist, d_idx);
            else if (rows == 2) mtf_ts_launch<Acc, 2>(ctx, acc, N, lut, al.sigma, ts, ts_seg, ts_flist, d_idx);
            else if (rows == 3) mtf_ts_launch<Acc, 3>(ctx, acc, N, lut, al.sigma, ts, ts_seg, ts_flist, d_idx);
            else if (rows == 4) mtf_ts_launch<Acc, 4>(ctx, acc, N, lut, al.sigma, ts, ts_seg, ts_flist, d_idx);
            else mtf_ts_launch<Acc, 5>(ctx, acc, N, lut, al.sigma, ts, ts_seg, ts_flist, d_idx);
            std::vector<u16> fl(al.sigma);
            tc_d2h(ctx, fl.data(), ts_flist, fl.size() * sizeof(u16));
            TC_HIP(ctx, hipStreamSynchronize(s));
            for (u32 i = 0; i < al.sigma; i++) final_list[i] = al.sym_of_code[fl[i]];
            return;
        }
        // large alphabets: lane chunks unless the sampled average rank says the symbols are spread
        // uniformly (tc_mtf.hpp, "which general path?")
        auto prefers_wave = [&](const Alphabet &ax) {
            if (ax.sigma <= 128 || N < (u64)MRS_BLOCKS * 256 * MRS_WIN || env_int("TC_MTF_RANK_SAMPLE", 1) == 0)
                return false;
            u64 *d_sum = ctx->d_scalars + 23;
            tc_memset_async(ctx, d_sum, 0, sizeof(u64));
            mtf_rank_sample_kernel<Acc><<<MRS_BLOCKS, 256, 0, s>>>(acc, N, d_sum);
            TC_LAUNCH_CHECK(ctx);
            tc_d2h(ctx, &ctx->h_scalars[23], d_sum, sizeof(u64));
            TC_HIP(ctx, hipStreamSynchronize(s));
            const u64 avg = ctx->h_scalars[23] / ((u64)MRS_BLOCKS * 256);   // distinct symbols per window
            return avg >= (u64)env_int("TC_MTF_WAVE_MIN_DISTINCT", 128);
        };
        if constexpr (std::is_same<Acc, BwtAcc>::value) {
            // sigma = 257 with the one sentinel of a BWT: 256-symbol lane chunks + fix-ups (tc_mtf.hpp)
            u32 bytes_only[257];
            memcpy(bytes_only, counts257, sizeof bytes_only);
            bytes_only[0] = 0;
            Alphabet ab;
            ab.build(bytes_only);   // 256 symbols, code = byte value
            if (al.sigma == 257 && acc.primary > 0 && (u64)acc.primary < N &&
                env_int("TC_MTF_WAVE_CHUNKS", 0) == 0 && env_int("TC_MTF_SENTINEL_SPLIT", 1) != 0 &&
                !prefers_wave(ab)) {
                BwtAcc dup = acc;
                dup.dup = 1;
                mtf_lane_launch<BwtAcc, 4>(ctx, dup, N, ab, lists, seen, d_idx);
                u32 *first = t_mask;    // 512 words (tiles + 1 >= 1: sized below)
                tc_memset_async(ctx, first, 0xff, 512 * sizeof(u32));
                u32 grid = tc_cdiv(N, 256 * 64);
                if (grid > 4096) grid = 4096;
                mtf257_first_kernel<<<grid, 256, 0, s>>>(acc.L, N, (u64)acc.primary, first);
                TC_LAUNCH_CHECK(ctx);
                mtf257_fix_kernel<<<1, 512, 0, s>>>(d_idx, first, (u64)acc.primary, ctx->d_scalars + 20);
                TC_LAUNCH_CHECK(ctx);
                std::vector<u16> fl(256);
                tc_d2h(ctx, fl.data(), lists + (size_t)tc_cdiv(N, GM_TILE) * 256, 256 * sizeof(u16));
                tc_d2h(ctx, &ctx->h_scalars[20], ctx->d_scalars + 20, 2 * sizeof(u64));
                TC_HIP(ctx, hipStreamSynchronize(s));
                const u32 after = (u32)ctx->h_scalars[21];   // distinct values met after the sentinel
                for (u32 i = 0, k = 0; i < 257; i++)
                    final_list[i] = i == after ? (i16)-1 : ab.sym_of_code[fl[k++]];
                return;
            }
        }
        if (al.sigma <= 256 && env_int("TC_MTF_WAVE_CHUNKS", 0) == 0 && !prefers_wave(al)) {
            rows = (int)((al.sigma + 63) / 64);
            last = tc_cdiv(N, GM_TILE);
            if (rows == 1) mtf_lane_launch<Acc, 1>(ctx, acc, N, al, lists, seen, d_idx);
            else if (rows == 2) mtf_lane_launch<Acc, 2>(ctx, acc, N, al, lists, seen, d_idx);
            else if (rows == 3) mtf_lane_launch<Acc, 3>(ctx, acc, N, al, lists, seen, d_idx);
            else mtf_lane_launch<Acc, 4>(ctx, acc, N, al, lists, seen, d_idx);
        } else {  // sigma = 257 (nine-bit codes): one chunk per wave
            rows = al.sigma <= 64 ? 1 : (al.sigma <= 128 ? 2 : 5);
            last = chunks;
            if (rows == 1) mtf_general_launch<Acc, 1>(ctx, acc, N, lut, lists, seen, chunks, d_idx);
            else if (rows == 2) mtf_general_launch<Acc, 2>(ctx, acc, N, lut, lists, seen, chunks, d_idx);
            else mtf_general_launch<Acc, 5>(ctx, acc, N, lut, lists, seen, chunks, d_idx);
        }
        std::vector<u16> fl(rows * 64);
        tc_d2h(ctx, fl.data(), lists + (size_t)last * (rows * 64), fl.size() * sizeof(u16));
        TC_HIP(ctx, hipStreamSynchronize(s));
        for (u32 i = 0; i < al.sigma; i++) final_list[i] = al.sym_of_code[fl[i]];
    }
}

// ------------------------------------------------------------------------- RLE
template <class Acc, class SymT>
static void rle_encode_device(tc_ctx *ctx, Arena &A, Acc acc, u64 N, u32 *d_counts, SymT *d_syms,
                              u64 cap, u64 *total, bool dry, bool small16 = false /* values < 16 (byte-wide stream) */) {
    const bool idx_stream = std::is_same<Acc, U16Acc>::value || std::is_same<Acc, U8Acc>::value;
    const u32 tiles = tc_cdiv(N, idx_stream ? RLE16_TILE : RLE_TILE);
    const u32 btiles = tc_cdiv(N, RN_TILE);                     // tiles of the blocked kernel (byte-wide index stream)
    const u32 stiles = tiles > btiles ? tiles : btiles;
    u64 *status = A.get<u64>(2 * (size_t)stiles + 4);
    if (dry) return;
    tc_memset_async(ctx, status, 0, (2 * (size_t)stiles + 4) * sizeof(u64));
    if constexpr (std::is_same<Acc, U8Acc>::value) {
        // byte-wide index stream (the fused encode): the blocked kernel (tc_pack.hpp); TC_RLE_BLOCKED=0: the striped one
        if ((((uintptr_t)acc.v) & 15) == 0 && env_int("TC_RLE_BLOCKED", 1) != 0) {
            RleBlkArgs b;
            b.src = acc.v; b.N = N; b.counts = d_counts; b.vals = reinterpret_cast<u16 *>(d_syms); b.cap = cap;
            b.status_a = status; b.status_b = status + btiles;
            b.ticket = reinterpret_cast<u32 *>(status + 2 * (size_t)btiles);
            b.scalars = ctx->d_scalars; b.err = ctx->d_err; b.ntiles = btiles;
            b.wide = ((((uintptr_t)d_counts) | ((uintptr_t)d_syms)) & 15) == 0 ? 1u : 0u;
            if (small16) {    // (values < 16: one staged byte per run)
                u32 grid = tc_persistent_grid_for(ctx, rle_blk_kernel<true>, RN_NT, 8);
                if (grid > btiles) grid = btiles;
                rle_blk_kernel<true><<<grid, RN_NT, 0, ctx->stream>>>(b);
            } else {
                u32 grid = tc_persistent_grid_for(ctx, rle_blk_kernel<false>, RN_NT, 8);
                if (grid > btiles) grid = btiles;
                rle_blk_kernel<false><<<grid, RN_NT, 0, ctx->stream>>>(b);
            }
            TC_LAUNCH_CHECK(ctx);
            tc_d2h(ctx, &ctx->h_scalars[2], ctx->d_scalars + 2, sizeof(u64));
            TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            *total = ctx->h_scalars[2];
            return;
        }
    }
    RleArgs a;
    a.N = N; a.counts = d_counts; a.syms = d_syms; a.cap = cap;
    a.status_pair = status; a.status_sum = status + tiles;
    a.ticket = reinterpret_cast<u32 *>(status + 2 * (size_t)tiles);
    a.scalars = ctx->d_scalars; a.err = ctx->d_err;
    a.diag = env_int("TC_RLE_DIAG", 0);
    if constexpr (std::is_same<Acc, U16Acc>::value) {
        u32 grid = tc_persistent_grid_for(ctx, rle_encode_idx_kernel<u16>, RLE_NT, 2);
        if (grid > tiles) grid = tiles;
        rle_encode_idx_kernel<u16><<<grid, RLE_NT, 0, ctx->stream>>>(acc.v, a);
    } else if constexpr (std::is_same<Acc, U8Acc>::value) {
        u32 grid = tc_persistent_grid_for(ctx, rle_encode_idx_kernel<u8>, RLE_NT, 2);
        if (grid > tiles) grid = tiles;
        rle_encode_idx_kernel<u8><<<grid, RLE_NT, 0, ctx->stream>>>(acc.v, a);
    } else {
        u32 grid = tc_persistent_grid_for(ctx, rle_encode_kernel<Acc, SymT>, RLE_NT, 2);
        if (grid > tiles) grid = tiles;
        rle_encode_kernel<Acc, SymT><<<grid, RLE_NT, 0, ctx->stream>>>(acc, a);
    }
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[2], ctx->d_scalars + 2, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *total = ctx->h_scalars[2];
}

// seqToMTF and seqToRLE of a last column over at most 8 symbols in one kernel (tc_pack.hpp, mtf_rle_kernel): the
// index stream is never written.  false (nothing written that matters): another alphabet, unaligned run arrays, or a
// tile whose incoming list the backward scan did not recover -- the caller runs the two stages.  TC_MTF_RLE=0: never.
static bool mtf_rle_device(tc_ctx *ctx, Arena &A, BwtAcc acc, u64 N, const u32 *counts257, tc_block *out, u64 cap,
                           u64 *total, u32 *sigma, bool dry) {
    const u32 tiles = tc_cdiv(N, MTF_TILE);
    u64 *status = A.get<u64>(2 * (size_t)tiles + 8);
    if (dry || env_int("TC_MTF_RLE", 1) == 0 || env_int("TC_MTF_FORCE_GENERAL", 0) != 0) return false;
    Alphabet al;
    al.build(counts257);
    if (al.sigma > 8 || N + 64 >= (1ull << 32)) return false;
    hipStream_t s = ctx->stream;
    MtfRleArgs a;
    for (int v = 0; v < 257; v++) a.lut.v[v] = (u8)al.code_of_sym[v];
    tc_memset_async(ctx, status, 0, (2 * (size_t)tiles + 8) * sizeof(u64));
    a.acc = acc; a.N = N; a.sigma = al.sigma;
    a.flag = reinterpret_cast<u32 *>(status + 2 * (size_t)tiles + 1);
    a.counts = out->run_count; a.vals = reinterpret_cast<u16 *>(out->run_value); a.cap = cap;
    a.status_a = status; a.status_b = status + tiles;
    a.ticket = reinterpret_cast<u32 *>(status + 2 * (size_t)tiles);
    a.scalars = ctx->d_scalars; a.err = ctx->d_err; a.ntiles = tiles;
    a.wide = ((((uintptr_t)out->run_count) | ((uintptr_t)out->run_value)) & 15) == 0 ? 1u : 0u;
    mtf_rle_kernel<false><<<tiles, MTF_NT, 0, s>>>(a);
    TC_LAUNCH_CHECK(ctx);
    u64 *d_final = status + 2 * (size_t)tiles + 2;
    mtf_nib_final_kernel<BwtAcc><<<1, 64, 0, s>>>(acc, N, a.lut, al.sigma, d_final, a.flag);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[15], a.flag, sizeof(u32));
    tc_d2h(ctx, &ctx->h_scalars[8], d_final, sizeof(u64));
    tc_d2h(ctx, &ctx->h_scalars[2], ctx->d_scalars + 2, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
#ifdef MTFRLE_PROFILE
    {
        u64 h[9];
        tc_d2h(ctx, h, ctx->d_scalars + 112, sizeof h);
        TC_HIP(ctx, hipStreamSynchronize(s));
        const double c = (double)(h[8] | 1);
        fprintf(stderr, "mtf_rle: tiles %llu | cycles per tile: stage+B %.0f pass %.0f scan+replay+B %.0f ends+B %.0f lookback A/counts+B %.0f lookback B+B %.0f emit+B %.0f copy-out %.0f\n",
                (unsigned long long)h[8], h[0] / c, h[1] / c, h[2] / c, h[3] / c, h[4] / c, h[5] / c, h[6] / c, h[7] / c);
        tc_memset_async(ctx, ctx->d_scalars + 112, 0, sizeof h);
    }
#endif
    if ((u32)ctx->h_scalars[15] != 0) {
        ctx->mtf_fastin_failed = 1;
        return false;
    }
    const u64 perm = ctx->h_scalars[8];
    for (u32 i = 0; i < al.sigma; i++) out->final_list[i] = al.sym_of_code[(perm >> (4 * i)) & 15];
    *sigma = al.sigma;
    *total = ctx->h_scalars[2];
    return true;
}

// --------------------------------------------------------------- fused pipeline
// The front of a fused encode, dry or for real: carves the last column and the index stream (N + idx_pad
// elements: what the caller's later stages read behind it), sorts the suffixes between events 0 and 1, and
// rewinds the arena to behind the two -- the suffix-sort buffers are dead, MTF / RLE scratch overlays them.
// Returns the accessor of the last column.
static BwtAcc encode_sa_stage(tc_ctx *ctx, Arena &A, bool dry, const u8 *d_text, u64 n, u64 idx_pad, u16 **d_idx,
                              u64 *primary, u32 *counts257) {
    const u64 N = n + 1;
    u32 counts[256];
    u8 *d_L = A.get<u8>(N + 16);
    *d_idx = A.get<u16>(N + idx_pad);
    const size_t mark = A.off;
    if (!dry) TC_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    sa_build(ctx, A, d_text, n, nullptr, d_L, primary, counts, dry);
    A.rewind(mark);
    if (!dry) {
        TC_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
        counts257[0] = 1;
        for (int b = 0; b < 256; b++) counts257[1 + b] = counts[b];
    }
    return BwtAcc{d_L, (i64)*primary};
}
// the stage times of a fused encode, from events 0 .. 3 (recorded, and the stream synchronised)
static void encode_stage_times(tc_ctx *ctx) {
    tc_stats &st = ctx->stats;
    (void)hipEventElapsedTime(&st.ms_sa, ctx->ev[0], ctx->ev[1]);
    (void)hipEventElapsedTime(&st.ms_mtf, ctx->ev[1], ctx->ev[2]);
    (void)hipEventElapsedTime(&st.ms_rle, ctx->ev[2], ctx->ev[3]);
    (void)hipEventElapsedTime(&st.ms_total, ctx->ev[0], ctx->ev[3]);
    st.ms_bwt = 0;  // the last column is produced inside the suffix-sort kernels
}

// bytestringToBWT -> bytestringBWTToMTFB -> runs of the index stream.
static void encode_device(tc_ctx *ctx, const u8 *d_text, u64 n, tc_block *out, u64 cap) {
    const u64 N = n + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    u64 primary = 0, total = 0;
    u32 counts257[257];
    u32 sigma = 0;
    hipStream_t s = ctx->stream;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool dry) {
        u16 *d_idx = nullptr;
        BwtAcc acc = encode_sa_stage(ctx, A, dry, d_text, n, 0, &d_idx, &primary, counts257);
        // small alphabets: the index stream between the two stages is one byte per symbol (the
        // same buffer, half used)
        bool idx8 = false;
        if (mtf_rle_device(ctx, A, acc, N, counts257, out, cap, &total, &sigma, dry)) {   // (sigma <= 8: one kernel)
            TC_HIP(ctx, hipEventRecord(ctx->ev[2], s));
            TC_HIP(ctx, hipEventRecord(ctx->ev[3], s));
            return;
        }
        mtf_encode_device<BwtAcc>(ctx, A, acc, N, dry ? nullptr : counts257, d_idx,
                                  out->final_list, &sigma, dry, reinterpret_cast<u8 *>(d_idx), &idx8);
        if (!dry) TC_HIP(ctx, hipEventRecord(ctx->ev[2], s));
        if (idx8) {
            U8Acc iacc{reinterpret_cast<const u8 *>(d_idx)};
            rle_encode_device<U8Acc, u16>(ctx, A, iacc, N, out->run_count, out->run_value, cap, &total, dry, sigma <= 16);
        } else {
            U16Acc iacc{d_idx};
            rle_encode_device<U16Acc, u16>(ctx, A, iacc, N, out->run_count, out->run_value, cap, &total, dry);
        }
        if (!dry) TC_HIP(ctx, hipEventRecord(ctx->ev[3], s));
    });
    tc_sync_check(ctx);
    out->n = n; out->primary = primary; out->sigma = sigma; out->nruns = total;
    ctx->stats.runs = total;
    encode_stage_times(ctx);
    if (total > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu run slots, have %llu",
                             (unsigned long long)total, (unsigned long long)cap);
}
