// tc_esa_xdoc.hpp -- cross-document matches on the kept enhanced suffix array: for every position of a collection the longest
// match that starts in another (or an earlier) document, where its copy is, and per document the bytes shared and the longest
// match (included by tc_esa_xdoc_host.hpp behind tc_esa_docs_host.hpp; it uses the min tree, the row searches of tc_fm_ms.hpp
// and the range minimum of tc_lz.hpp unchanged).  No counterpart in the reference.
// host/check/esx_kernels.cpp compiles both instances of esx_match_kernel and the lane bodies of the scans and of the
// per-document sums -- esx_bmask, esx_lane_heads, esx_seg_join, esx_seg_lane, esx_lane_sum, esx_lower -- as plain C++
// (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes); the workgroup scans and the tile kernels around the lane bodies exist on the
// device only.
//
// include/textcomp.h defines the answers.  Over the N = n + 1 rows of a handle with documents (da[r] = the document of sa[r]):
//   OTHER    row r >= 1 is a BOUNDARY iff da[r] != da[r - 1] (row 1 always is: da[0] is no document).  The rows between two
//            boundaries are a run of one document, so the nearest row above r of another document is (the last boundary at or
//            before r) - 1 -- row 0, which never qualifies, where that boundary is row 1 -- and the nearest below is the first
//            boundary behind r.  up[r] and dn[r] hold both: a max scan and a reverse min scan over tiles of ESX_TILE rows
//            (esx_reduce_kernel: each tile's last and first boundary; sus_spine_kernel of tc_sus.hpp, unchanged: the exclusive
//            prefix maximum and suffix minimum over the tiles; esx_heads_kernel: the scan within the tile).  No lane walks a
//            run: one document, one run over every tile, costs the passes of 65535 documents.
//   EARLIER  the nearest rows above and below r with da < da[r]: fm_ms_prev_below / fm_ms_next_below over a min tree of da
//            that the call builds in its workspace.  da[0] = 0xffffffff is below nothing, and the downward search answers 0
//            where it finds nothing: 0 is "no row" either way.
//   match    esx_match_kernel, one lane per row r >= 1: the two neighbours a < r < b, La = min lcp(a, r], Lb = min lcp(r, b]
//            (lcp[r] and lcp[r + 1] where the neighbour is adjacent, else one lz_range_min each: at most 2 f words per level),
//            the better of the two (a on a tie), the clamp from doc_start[da[r] + 1], and three scattered stores at sa[r].
//   shared   the clamped lengths go to the workspace; the cover core of tc_cov.hpp, unchanged (cov_reduce_kernel,
//            cov_spine_kernel, cov_mask_kernel without a map), makes the 0/1 cover of them; esx_tile_sum_kernel sums the
//            cover per tile of ESX_STILE bytes, tc_scan64 gives every tile's prefix, esx_doc_prefix_kernel adds the partial
//            tile before each of the ndocs + 1 boundaries (one workgroup per boundary, at most one tile read), and
//            esx_doc_diff_kernel subtracts neighbours.
//   longest  a segmented maximum, the segments starting at the documents' first positions: esx_seg_kernel<0> gives every tile
//            of ESX_TILE positions its (a segment starts here, the maximum behind the last start) pair, esx_seg_spine_kernel
//            the segmented exclusive scan of the pairs in one workgroup, esx_seg_kernel<1> the segmented scan within the tile
//            into LDS, where the documents that END in the tile read their answer at their last position.  The tile finds its
//            documents by one binary search in doc_start; its lanes stride over them.  No lane or workgroup walks a document.
// No atomics reach global memory: two calls give identical output.  Every index read from up, dn, da or a tree is checked
// against the row count before it is used, so arrays of arbitrary contents keep every access in bounds.
#pragma once
#include "tc_esa_docs.hpp"
#ifndef TC_FM_MS_HOST_CHECK
#include "tc_sus.hpp"
#include "tc_cov.hpp"
#endif

#define ESX_OTHER 0             // TC_DOC_OTHER of include/textcomp.h
#define ESX_EARLIER 1           // TC_DOC_EARLIER
#define ESX_NO_POS 0xffffffffu  // TC_ESA_NO_POS
#define ESX_NT 256
#define ESX_ROWS 8
#define ESX_TILE 2048           // = ESX_NT * ESX_ROWS rows (the heads) or positions (the segmented maximum) per workgroup; tests/test_gpu_doc_match.py states the same number
#define ESX_SBYTES 16
#define ESX_STILE 4096          // = ESX_NT * ESX_SBYTES cover bytes per tile of the per-document sums

#ifdef TC_FM_MS_HOST_CHECK
// what host/check/esx_kernels.cpp asserts happened: [0] no qualifying row above, [1] none below, [2] neither, [3] the clamp
// fired, [4] the neighbour above was adjacent, [5] the one below was, [6] a range minimum above, [7] below, [8] a row skipped
// (not on a suffix or document array), [9] a neighbour out of range dropped
static u64 esx_seen[10] = {};
#define ESX_SEEN(k) (esx_seen[k]++)
#else
#define ESX_SEEN(k) ((void)0)
#endif

// ---- the lane bodies
// bit k: row base + k is a boundary.  w[k] = da[base + k - 1], k = 0 .. ESX_ROWS (entries of rows outside [0, N) are not looked at)
FM_MS_HD u32 esx_bmask(const u32 *w, u64 base, u64 N) {
    u32 m = 0;
    for (u32 k = 0; k < ESX_ROWS; k++) {
        const u64 r = base + k;
        if (r >= 1 && r < N && w[k + 1] != w[k]) m |= 1u << k;
    }
    return m;
}
// the last boundary of the mask, + 1 (0: none); the first (N: none)
FM_MS_HD u32 esx_last1(u32 mask, u64 base) { return mask ? (u32)(base + (31u - (u32)__builtin_clz(mask)) + 1u) : 0u; }
FM_MS_HD u32 esx_first(u32 mask, u64 base, u32 N) { return mask ? (u32)(base + (u32)__builtin_ctz(mask)) : N; }
// up and dn of the lane's rows below N.  prev1: the last boundary before the lane's rows, + 1 (0: none); next: the first
// boundary behind them (N: none)
FM_MS_HD void esx_lane_heads(u32 mask, u64 base, u64 N, u32 prev1, u32 next, u32 *up, u32 *dn) {
    u32 h1 = prev1;
    for (u32 k = 0; k < ESX_ROWS; k++) {
        const u64 r = base + k;
        if (r >= N) break;
        if ((mask >> k) & 1u) h1 = (u32)r + 1u;
        up[r] = h1 >= 2u ? h1 - 2u : 0u;        // (the head of r) - 1; 0: no row above (row 0 never qualifies)
    }
    u32 nx = next;
    for (u32 k = ESX_ROWS; k-- > 0;) {
        const u64 r = base + k;
        if (r >= N) continue;
        dn[r] = nx;
        if ((mask >> k) & 1u) nx = (u32)r;
    }
}

// the smallest j in [0, ndocs] with ds[j] >= x, ndocs + 1 where there is none (ds: doc_start, ndocs + 1 entries, non-decreasing)
FM_MS_HD u32 esx_lower(const u32 *ds, u32 ndocs, u64 x) {
    u32 lo = 0, hi = ndocs + 1u;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (ds[mid] >= x) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// A value of the segmented maximum: (a segment starts at or before here) << 32 | the maximum since.  a stands before b.
FM_MS_HD u64 esx_seg_join(u64 a, u64 b) {
    if (b >> 32) return b;
    const u32 x = (u32)a, y = (u32)b;
    return (a & ~0xffffffffull) | (x > y ? x : y);
}
// the lane's ESX_ROWS positions behind `acc`: v their values, bit k of starts: a document starts at position k; out (may be
// null) receives the running maximum at each position
FM_MS_HD u64 esx_seg_lane(u64 acc, const u32 *v, u32 starts, u32 *out) {
    for (u32 k = 0; k < ESX_ROWS; k++) {
        acc = esx_seg_join(acc, (u64)((starts >> k) & 1u) << 32 | v[k]);
        if (out) out[k] = (u32)acc;
    }
    return acc;
}

// the sum of cov[from .. min(from + ESX_SBYTES, to))
FM_MS_HD u32 esx_lane_sum(const u8 *cov, u64 from, u64 to) {
    u32 s = 0;
    for (u32 k = 0; k < ESX_SBYTES; k++)
        if (from + k < to) s += cov[from + k];
    return s;
}

// ---- the match: one lane per row r >= 1.  KIND = ESX_OTHER reads up and dn, ESX_EARLIER the min tree da_min of da.  xl, src
// and xdoc (each may be null) are stored at position sa[r].
template <int KIND>
FM_MS_KERNEL esx_match_kernel(u32 n, const u32 *__restrict__ sa, const u32 *__restrict__ lcp, const u32 *__restrict__ lcp_min,
                              const u32 *__restrict__ da, const u32 *__restrict__ da_min, const u32 *__restrict__ up,
                              const u32 *__restrict__ dn, const u32 *__restrict__ doc_start, u32 ndocs, u32 lf, u32 clamp,
                              u32 *__restrict__ xl, u32 *__restrict__ src, u32 *__restrict__ xdoc) {
    const u32 N = n + 1u;
    ESA_TREE_SHAPE(N, lf);
    const u64 r64 = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid() + 1u;
    if (r64 >= N) return;
    const u32 r = (u32)r64, i = sa[r], d = da[r];
    if (i >= n || d >= ndocs) {                 // (not on a suffix array and its document array: rows 1 .. n hold 0 .. n - 1)
        ESX_SEEN(8);
        return;
    }
    FmMsTree L;
    L.lcp = lcp; L.lmin = lcp_min; L.s_off = s_off; L.s_cnt = s_cnt; L.nlev = s_nlev; L.lf = lf;
    u32 a = 0, b = N;                           // 0 / N: no qualifying row above / below
    if (KIND == ESX_OTHER) {
        a = up[r];
        b = dn[r];
    } else if (d) {                             // (the searches need a threshold >= 1; nothing is earlier than document 0)
        FmMsTree D = L;
        D.lcp = da; D.lmin = da_min;
        a = fm_ms_prev_below(D, r - 1u, d);
        b = fm_ms_next_below(D, N, r, d);
    }
    if (a >= r || b <= r || b > N) {            // (not from these arrays: keeps every row read below in [1, N))
        ESX_SEEN(9);
        if (a >= r) a = 0;
        if (b <= r || b > N) b = N;
    }
    const bool ha = a != 0, hb = b < N;
    u32 la = 0, lb = 0;
    if (ha) {
        if (a == r - 1u) {
            ESX_SEEN(4);
            la = lcp[r];
        } else {
            ESX_SEEN(6);
            la = lz_range_min<7>(L, a + 1u, r);
        }
    }
    if (hb) {
        if (b == r + 1u) {
            ESX_SEEN(5);
            lb = lcp[b];
        } else {
            ESX_SEEN(7);
            lb = lz_range_min<7>(L, r + 1u, b);
        }
    }
    if (!ha) ESX_SEEN(hb ? 0 : 2);
    else if (!hb) ESX_SEEN(1);
    const bool take_a = ha && (!hb || la >= lb);
    const u32 p = take_a ? a : b;
    u32 l = take_a ? la : (hb ? lb : 0u);
    u32 s = ESX_NO_POS, sd = ESD_NO_DOC;
    if (l) {
        s = sa[p];
        sd = da[p];
        if (clamp) {
            const u32 e = doc_start[d + 1u], room = e > i ? e - i : 0u;
            if (room < l) {
                ESX_SEEN(3);
                l = room;
            }
        }
    }
    if (xl) xl[i] = l;
    if (src) src[i] = s;
    if (xdoc) xdoc[i] = sd;
}

#ifndef TC_FM_MS_HOST_CHECK
// the lane's da words: w[k] = da[base + k - 1], k = 0 .. ESX_ROWS (0 outside the array)
__device__ __forceinline__ void esx_load_da(const u32 *__restrict__ da, u64 base, u64 N, u32 *w) {
#pragma unroll
    for (u32 k = 0; k <= ESX_ROWS; k++) {
        const u64 r1 = base + k;                // row + 1
        w[k] = r1 >= 1 && r1 <= N ? da[r1 - 1u] : 0u;
    }
}

// tlast[t] = the last boundary row of tile t, + 1 (0: none); tfirst[t] = its first boundary row (N: none)
__global__ __launch_bounds__(ESX_NT, 8) void esx_reduce_kernel(const u32 *__restrict__ da, u32 N, u32 *__restrict__ tlast,
                                                               u32 *__restrict__ tfirst) {
    __shared__ u32 s_max[ESX_NT / 64], s_min[ESX_NT / 64];
    const u64 base = (u64)blockIdx.x * ESX_TILE + (u64)threadIdx.x * ESX_ROWS;
    u32 w[ESX_ROWS + 1];
    esx_load_da(da, base, N, w);
    const u32 mask = esx_bmask(w, base, N);
    u32 hi = esx_last1(mask, base), lo = esx_first(mask, base, N);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 x = __shfl_xor(hi, d, 64), y = __shfl_xor(lo, d, 64);
        hi = x > hi ? x : hi;
        lo = y < lo ? y : lo;
    }
    if ((threadIdx.x & 63) == 0) {
        s_max[threadIdx.x >> 6] = hi;
        s_min[threadIdx.x >> 6] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 i = 1; i < ESX_NT / 64; i++) {
            hi = s_max[i] > hi ? s_max[i] : hi;
            lo = s_min[i] < lo ? s_min[i] : lo;
        }
        tlast[blockIdx.x] = hi;
        tfirst[blockIdx.x] = lo;
    }
}

// up[r] and dn[r] of every row; tlast / tfirst: the tiles' carries (sus_spine_kernel over esx_reduce_kernel's)
__global__ __launch_bounds__(ESX_NT, 8) void esx_heads_kernel(const u32 *__restrict__ da, u32 N, const u32 *__restrict__ tlast,
                                                              const u32 *__restrict__ tfirst, u32 *__restrict__ up, u32 *__restrict__ dn) {
    __shared__ u32 s_max[ESX_NT / 64], s_min[ESX_NT / 64];
    const u64 base = (u64)blockIdx.x * ESX_TILE + (u64)threadIdx.x * ESX_ROWS;
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    u32 w[ESX_ROWS + 1];
    esx_load_da(da, base, N, w);
    const u32 mask = esx_bmask(w, base, N);
    u32 imax = esx_last1(mask, base), imin = esx_first(mask, base, N);      // inclusive over the wave: up to this lane, from it on
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 x = __shfl_up(imax, d, 64), y = __shfl_down(imin, d, 64);
        if ((int)lane >= d) imax = x > imax ? x : imax;
        if ((int)lane + d < 64) imin = y < imin ? y : imin;
    }
    if (lane == 63) s_max[wv] = imax;
    if (lane == 0) s_min[wv] = imin;
    u32 prev1 = __shfl_up(imax, 1, 64), next = __shfl_down(imin, 1, 64);
    if (lane == 0) prev1 = 0;
    if (lane == 63) next = N;
    __syncthreads();
    const u32 t0 = tlast[blockIdx.x], t1 = tfirst[blockIdx.x];
    prev1 = t0 > prev1 ? t0 : prev1;
    next = t1 < next ? t1 : next;
#pragma unroll
    for (u32 i = 0; i < ESX_NT / 64; i++) {
        if (i < wv) prev1 = s_max[i] > prev1 ? s_max[i] : prev1;
        if (i > wv) next = s_min[i] < next ? s_min[i] : next;
    }
    esx_lane_heads(mask, base, N, prev1, next, up, dn);
}

// ---- the per-document sums
// tsum[t] = the sum of the cover bytes of tile t (the grid has one tile behind the last: it sums to 0)
__global__ __launch_bounds__(ESX_NT, 8) void esx_tile_sum_kernel(const u8 *__restrict__ cov, u64 n, u64 *__restrict__ tsum) {
    __shared__ u32 s_sum[ESX_NT / 64];
    const u64 from = (u64)blockIdx.x * ESX_STILE + (u64)threadIdx.x * ESX_SBYTES;
    const u32 v = wave_sum(esx_lane_sum(cov, from, n));
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 s = 0;
        for (u32 i = 0; i < ESX_NT / 64; i++) s += s_sum[i];
        tsum[blockIdx.x] = s;
    }
}
// One workgroup per boundary j = 0 .. ndocs: pre[j] = the covered bytes before doc_start[j] = tbase[its tile] + the tile's
// bytes before it
__global__ __launch_bounds__(ESX_NT, 8) void esx_doc_prefix_kernel(const u8 *__restrict__ cov, u64 n, const u32 *__restrict__ doc_start,
                                                                   const u64 *__restrict__ tbase, u64 *__restrict__ pre) {
    __shared__ u32 s_sum[ESX_NT / 64];
    const u64 p = doc_start[blockIdx.x] < n ? doc_start[blockIdx.x] : n;
    const u64 t = p / ESX_STILE, from = t * ESX_STILE + (u64)threadIdx.x * ESX_SBYTES;
    const u32 v = wave_sum(esx_lane_sum(cov, from, p));
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 s = 0;
        for (u32 i = 0; i < ESX_NT / 64; i++) s += s_sum[i];
        pre[blockIdx.x] = tbase[t] + s;
    }
}
// shared[d] = pre[d + 1] - pre[d]
__global__ __launch_bounds__(ESX_NT, 8) void esx_doc_diff_kernel(const u64 *__restrict__ pre, u32 ndocs, u64 *__restrict__ shared) {
    const u32 d = blockIdx.x * ESX_NT + threadIdx.x;
    if (d < ndocs) shared[d] = pre[d + 1u] - pre[d];
}

// ---- the segmented maximum
// workgroup exclusive scan of esx_seg_join (0 is the identity); smem: ESX_NT / 64 words.  *total = the join of all.
__device__ __forceinline__ u64 esx_block_excl_seg(u64 v, u64 *smem, u64 *total) {
    const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(inc, d, 64);
        if ((int)lane >= d) inc = esx_seg_join(t, inc);
    }
    u64 ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0;
    __syncthreads();
    if (lane == 63) smem[wv] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (u32 i = 0; i < ESX_NT / 64; i++) {
        const u64 s = smem[i];
        if (i < wv) base = esx_seg_join(base, s);
        tot = esx_seg_join(tot, s);
    }
    *total = tot;
    return esx_seg_join(base, ex);
}

// A tile of ESX_TILE positions of len[0 .. n).  PASS 0: pair[t] = the tile's value of the segmented maximum (a document
// starts in it, the maximum behind the last start).  PASS 1: pair[t] holds the value of everything before the tile (esx_seg_spine_kernel);
// longest[d] of every document whose last position lies in the tile.  (A document that ends at position 0 is empty: the host
// zeroes longest before.)
template <int PASS>
__global__ __launch_bounds__(ESX_NT, 8) void esx_seg_kernel(const u32 *__restrict__ len, u32 n, const u32 *__restrict__ doc_start, u32 ndocs,
                                                            u64 *__restrict__ pair, u32 *__restrict__ longest) {
    __shared__ u32 s_bits[ESX_TILE / 32];
    __shared__ u64 s_scan[ESX_NT / 64];
    __shared__ u32 s_m[PASS ? ESX_TILE : 1];
    const u64 tb = (u64)blockIdx.x * ESX_TILE, te = tb + ESX_TILE, base = tb + (u64)threadIdx.x * ESX_ROWS;
    if (threadIdx.x < ESX_TILE / 32) s_bits[threadIdx.x] = 0;
    __syncthreads();
    for (u32 d = esx_lower(doc_start, ndocs, tb) + threadIdx.x; d < ndocs; d += ESX_NT) {      // the documents that start in the tile
        const u64 s = doc_start[d];
        if (s >= te) break;
        if (s >= tb) atomicOr(&s_bits[(u32)(s - tb) >> 5], 1u << ((u32)(s - tb) & 31u));
    }
    __syncthreads();
    u32 v[ESX_ROWS];
#pragma unroll
    for (u32 k = 0; k < ESX_ROWS; k++) v[k] = base + k < n ? len[base + k] : 0u;
    const u32 starts = (s_bits[threadIdx.x >> 2] >> ((threadIdx.x & 3u) * ESX_ROWS)) & ((1u << ESX_ROWS) - 1u);
    u64 total;
    const u64 before = esx_block_excl_seg(esx_seg_lane(0, v, starts, nullptr), s_scan, &total);
    if (PASS == 0) {
        if (threadIdx.x == 0) pair[blockIdx.x] = total;
        return;
    }
    u32 m[ESX_ROWS];
    esx_seg_lane(esx_seg_join(pair[blockIdx.x], before), v, starts, m);
#pragma unroll
    for (u32 k = 0; k < ESX_ROWS; k++) s_m[threadIdx.x * ESX_ROWS + k] = m[k];
    __syncthreads();
    for (u32 j = esx_lower(doc_start, ndocs, tb + 1u) + threadIdx.x; j <= ndocs; j += ESX_NT) {     // the boundaries in (tb, te]
        const u64 e = doc_start[j];
        if (e > te || e > n || j == 0) break;
        const u64 s = doc_start[j - 1u];
        longest[j - 1u] = s < e && e > tb ? s_m[(u32)(e - 1u - tb)] : 0u;
    }
}

// single workgroup, in place: pair[t] = the join of the tiles before t (0 for t = 0)
__global__ __launch_bounds__(1024) void esx_seg_spine_kernel(u64 *pair, u32 tiles) {
    __shared__ u64 s_v[1024];
    const u32 per = (tiles + 1023u) / 1024u;
    const u32 lo = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
    u64 a = 0;
    for (u32 t = lo; t < hi; t++) a = esx_seg_join(a, pair[t]);
    s_v[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = 0;
        for (int i = 0; i < 1024; i++) {
            const u64 c = s_v[i];
            s_v[i] = run;
            run = esx_seg_join(run, c);
        }
    }
    __syncthreads();
    u64 run = s_v[threadIdx.x];
    for (u32 t = lo; t < hi; t++) {
        const u64 c = pair[t];
        pair[t] = run;
        run = esx_seg_join(run, c);
    }
}
#endif  // TC_FM_MS_HOST_CHECK
