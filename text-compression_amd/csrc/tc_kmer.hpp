// tc_kmer.hpp -- the k-mers of a text from its enhanced suffix array: the list, the abundance spectrum and the all-k
// profile (included by tc_kmer_host.hpp behind tc_rep_host.hpp).  No counterpart in the reference.
// host/check/kmer_kernels.cpp compiles the per-lane bodies -- km_mask16, km_close, km_lane_close, km_profile_bins -- as
// plain C++ (TC_KM_HOST_CHECK: the HIP keywords defined away); the loads, the workgroup scans and the atomics around them
// exist on the device only.
//
// N = n + 1 rows, sa / lcp as tc_lcp_array defines them; lcp[0] counts as 0 whatever the array holds, lcp[N] as 0.  For
// k >= 1 row q is a BOUNDARY iff lcp[q] < k, and so is the virtual row N.  A K-MER is the row interval [p, q) between two
// consecutive boundaries whose first row is long enough, sa[p] + k <= n (in 64 bits): occ = q - p, pos = sa[p], row = p,
// in increasing row -- the lexicographic order of the k-mers.  Filters: min_occ <= occ, and occ <= max_occ unless
// max_occ = 0.
//   text          k   sa                              lcp                             (row, pos, occ)
//   mississippi   2   11 10 7 4 1 0 9 8 6 3 5 2       0 0 1 1 4 0 0 1 0 2 1 3         (2,7,1) (3,4,2) (5,0,1) (6,9,1) (7,8,1) (8,6,2) (10,5,2)
//   aaabaab       2   7 0 4 1 5 2 6 3                 0 0 2 3 1 2 0 1                 (1,0,3) (4,5,2) (7,3,1)
//   aaabaab       1   as above                        as above                        (1,0,5) (6,6,2)
//   aaaaaa        2                                                                   (2,4,5)
// (mississippi: ip, is x2, mi, pi, pp, si x2, ss x2.)
//
// No lane walks.  A tile is KM_TILE = 256 lanes x 16 rows; the tiles cover the rows 0 .. N, the virtual row included.  A
// lane turns its 16 lcp words into a 16-bit boundary mask.  A group is closed at its END boundary q; its head p is the
// previous boundary: a lower bit of the lane's own mask, else the last boundary of an earlier lane of the tile (a
// workgroup exclusive max scan of the lanes' last boundary rows), else carry[t], the last boundary of any earlier tile.
// km_tile_kernel writes each tile's last boundary row (+ 1; 0: none) and km_carry_kernel max-scans those N / KM_TILE + 1
// words.  So a unary text, one k-mer over all rows, costs every lane its 16 rows and O(1), like any other text.
// Row 0 is always a boundary, so every q >= 1 has a head, and p < q <= N: sa[p] is the one read of sa per group, always in
// bounds, and its value is only copied and compared, never used as an index -- the passes stay in bounds on ANY contents
// of the two arrays.
#pragma once
#ifdef TC_KM_HOST_CHECK
#include <stdint.h>
typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
#define KM_HD static inline
#else
#define KM_HD __device__ __forceinline__
#endif

#define KM_NT 256
#define KM_ROWS 16
#define KM_TILE 4096            // = KM_NT * KM_ROWS rows per tile (tests/test_gpu_kmers.py states the same number)
#define KM_LDS_BINS 4096u       // spectrum bins kept in LDS: a tile closes at most KM_TILE groups, so u32 counters hold
#define KM_MAX_BINS 65536u
#define KM_MAX_KMAX 4096u
#define KM_PF_NT 512
#define KM_PF_ROWS 4
#define KM_PF_CHUNK (KM_PF_NT * KM_PF_ROWS)

// bit i: row base + i is a boundary.  w[i] = lcp[base + i] for the rows below N (the others are not looked at).
KM_HD u32 km_mask16(const u32 *w, u64 base, u64 N, u32 k) {
    u32 m = 0;
    for (u32 i = 0; i < KM_ROWS; i++) {
        const u64 r = base + i;
        const bool b = r == N || (r < N && (r == 0 || w[i] < k));
        m |= (b ? 1u : 0u) << i;
    }
    return m;
}
// the last boundary row of a mask, + 1; 0: none
KM_HD u32 km_last1(u32 mask, u64 base) { return mask ? (u32)(base + (31u - (u32)__builtin_clz(mask)) + 1u) : 0u; }

// the group [p, q), p < q, whose first suffix starts at sap: is it a k-mer that passes the filters?  *occ = q - p.
KM_HD bool km_close(u64 q, u64 p, u32 sap, u64 n, u32 k, u32 min_occ, u32 max_occ, u32 *occ) {
    const u64 o = q - p;
    *occ = (u32)o;
    return (u64)sap + (u64)k <= n && o >= min_occ && (max_occ == 0 || o <= max_occ);
}

// One lane: every boundary q of `mask` (rows base .. base + 15) closes the group that ends there.  prev1: the last boundary
// before the lane's rows, + 1 (0: none -- only row 0 itself has none).  emit(j, row, pos, occ) for the j-th k-mer that
// passes; returns how many did.  At most 16 turns, one read of sa each.
template <class F>
KM_HD u32 km_lane_close(u32 mask, u64 base, u32 prev1, const u32 *sa, u64 n, u32 k, u32 min_occ, u32 max_occ, F &&emit) {
    u32 c = 0;
    u64 p1 = prev1;
    while (mask) {
        const u32 i = (u32)__builtin_ctz(mask);
        mask &= mask - 1u;
        const u64 q = base + i;
        if (p1) {
            const u64 p = p1 - 1u;
            const u32 pos = sa[p];
            u32 occ;
            if (km_close(q, p, pos, n, k, min_occ, max_occ, &occ)) {
                emit(c, (u32)p, pos, occ);
                c++;
            }
        }
        p1 = q + 1u;
    }
    return c;
}

// the spectrum bin of a k-mer with occ occurrences: occ - 1, the last bin takes everything from `bins` on
KM_HD u32 km_spectrum_bin(u32 occ, u32 bins) { return (occ < bins ? occ : bins) - 1u; }

// The profile's two bins of row r < N, l = lcp[r], lnext = lcp[r + 1] (row 0 counts as 0, and so does row N):
// *a = min(l, kmax) counts towards #{r : lcp[r] >= k}, *b = min(max(l, lnext), kmax) towards the rows 1 .. n that are a
// group of their own at every k above it.  Returns whether *b counts (r >= 1).
KM_HD bool km_profile_bins(u64 r, u64 N, u32 l, u32 lnext, u32 kmax, u32 *a, u32 *b) {
    if (r == 0) l = 0;
    if (r + 1 >= N) lnext = 0;
    const u32 m = l > lnext ? l : lnext;
    *a = l < kmax ? l : kmax;
    *b = m < kmax ? m : kmax;
    return r >= 1;
}

#ifndef TC_KM_HOST_CHECK
enum { KM_COUNT = 0, KM_FILL = 1, KM_HIST = 2 };

// the lane's 16 lcp words: four 16-byte loads where the rows are all there and the array is 16-byte aligned
__device__ __forceinline__ void km_load16(const u32 *__restrict__ lcp, u64 base, u64 N, bool aligned, u32 *w) {
    if (aligned && base + KM_ROWS <= N) {
        const uint4 *v = reinterpret_cast<const uint4 *>(lcp + base);
#pragma unroll
        for (u32 i = 0; i < KM_ROWS / 4; i++) {
            const uint4 x = v[i];
            w[4 * i] = x.x; w[4 * i + 1] = x.y; w[4 * i + 2] = x.z; w[4 * i + 3] = x.w;
        }
    } else {
#pragma unroll
        for (u32 i = 0; i < KM_ROWS; i++) w[i] = base + i < N ? lcp[base + i] : 0u;
    }
}

// workgroup exclusive max scan of u32 (0 is the identity); smem: KM_NT / 64 words.  *total = the max of all.
__device__ __forceinline__ u32 km_block_excl_max(u32 v, u32 *smem, u32 *total) {
    const u32 w = threadIdx.x >> 6;
    const u32 inc = wave_incl_max(v);
    u32 ex = __shfl_up(inc, 1, 64);
    if (lane_id() == 0) ex = 0;
    __syncthreads();
    if (lane_id() == 63) smem[w] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (u32 i = 0; i < KM_NT / 64; i++) {
        const u32 s = smem[i];
        if (i < w) base = base > s ? base : s;
        tot = tot > s ? tot : s;
    }
    *total = tot;
    return ex > base ? ex : base;
}

// last[t] = the last boundary row of tile t, + 1; 0: the tile has none
__global__ __launch_bounds__(KM_NT) void km_tile_kernel(const u32 *__restrict__ lcp, u64 N, u32 k, u32 aligned, u32 *__restrict__ last) {
    __shared__ u32 s[KM_NT / 64];
    const u64 base = (u64)blockIdx.x * KM_TILE + (u64)threadIdx.x * KM_ROWS;
    u32 w[KM_ROWS];
    km_load16(lcp, base, N, aligned != 0, w);
    u32 v = km_last1(km_mask16(w, base, N, k), base);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 t = __shfl_xor(v, d, 64);
        v = v > t ? v : t;
    }
    if (lane_id() == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 m = 0;
        for (u32 i = 0; i < KM_NT / 64; i++) m = m > s[i] ? m : s[i];
        last[blockIdx.x] = m;
    }
}

// one workgroup: carry[t] = max last[0 .. t), the last boundary of any earlier tile (+ 1; 0: none)
__global__ __launch_bounds__(1024) void km_carry_kernel(const u32 *__restrict__ last, u32 *__restrict__ carry, u32 tiles) {
    __shared__ u32 s_part[1024];
    const u32 per = (tiles + 1023u) / 1024u;
    const u64 lo64 = (u64)threadIdx.x * per;
    const u32 lo = lo64 < tiles ? (u32)lo64 : tiles, hi = lo64 + per < tiles ? (u32)(lo64 + per) : tiles;
    u32 v = 0;
    for (u32 t = lo; t < hi; t++) v = v > last[t] ? v : last[t];
    s_part[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (u32 i = 0; i < 1024; i++) {
            const u32 c = s_part[i];
            s_part[i] = run;
            run = run > c ? run : c;
        }
    }
    __syncthreads();
    u32 run = s_part[threadIdx.x];
    for (u32 t = lo; t < hi; t++) {
        carry[t] = run;
        run = run > last[t] ? run : last[t];
    }
}

// The groups that END in tile t.  COUNT: cnt[t] = how many pass.  FILL: they go to pos / occ / row (row may be null) from
// slot offs[t] on, in row order: a workgroup scan of the lanes' counts, a pass through LDS, no atomics.  HIST: the abundance spectrum; the first
// min(bins, KM_LDS_BINS) bins are u32 counters in LDS, flushed by one 64-bit atomicAdd per non-zero bin, a group above that
// range (there are at most N / KM_TILE of them when bins > KM_LDS_BINS) adds to global memory itself; *distinct gets the
// tile's count.  (n = N - 1.)
template <int MODE>
__global__ __launch_bounds__(KM_NT) void km_pass_kernel(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, u64 N, u32 k,
                                                        u32 min_occ, u32 max_occ, u32 aligned, const u32 *__restrict__ carry,
                                                        u64 *__restrict__ cnt, const u64 *__restrict__ offs,
                                                        u32 *__restrict__ kpos, u32 *__restrict__ kocc, u32 *__restrict__ krow,
                                                        u64 *__restrict__ hist, u32 bins, u64 *__restrict__ distinct) {
    __shared__ u32 s_scan[KM_NT / 64 + 1];
    __shared__ u32 s_hist[MODE == KM_HIST ? KM_LDS_BINS : 1];
    __shared__ u32 s_stage[MODE == KM_FILL ? KM_TILE : 1];
    const u64 n = N - 1u;
    const u64 base = (u64)blockIdx.x * KM_TILE + (u64)threadIdx.x * KM_ROWS;
    const u32 lds_bins = bins < KM_LDS_BINS ? bins : KM_LDS_BINS;
    if (MODE == KM_HIST) {
        for (u32 i = threadIdx.x; i < lds_bins; i += KM_NT) s_hist[i] = 0;   // (the scan's barriers order this before the adds)
    }
    u32 w[KM_ROWS];
    km_load16(lcp, base, N, aligned != 0, w);
    const u32 mask = km_mask16(w, base, N, k);
    u32 tile_last;
    u32 prev1 = km_block_excl_max(km_last1(mask, base), s_scan, &tile_last);
    const u32 cr = carry[blockIdx.x];
    prev1 = prev1 > cr ? prev1 : cr;
    u32 c;
    if (MODE == KM_HIST) {
        u32 ones = 0;       // bin 0 is where most k-mers of a long k land: one add per wave, not one per k-mer
        c = km_lane_close(mask, base, prev1, sa, n, k, 1u, 0u, [&](u32, u32, u32, u32 occ) {
            const u32 b = km_spectrum_bin(occ, bins);
            if (b == 0) ones++;
            else if (b < lds_bins) atomicAdd(&s_hist[b], 1u);
            else atomicAdd(reinterpret_cast<unsigned long long *>(hist + b), 1ull);
        });
        ones = wave_sum(ones);
        if (lane_id() == 0 && ones) atomicAdd(&s_hist[0], ones);
    } else {
        c = km_lane_close(mask, base, prev1, sa, n, k, min_occ, max_occ, [](u32, u32, u32, u32) {});
    }
    u32 total;
    const u32 before = block_excl_sum<KM_NT>(c, s_scan, &total);
    if (MODE == KM_COUNT) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    } else if (MODE == KM_FILL) {
        // the tile's k-mers go through LDS, one packed word each, so that the three arrays are written -- and sa is read --
        // by consecutive lanes: the end q of a group lies in this tile, its head p does too or is the carry (0xffff)
        const u64 tile_base = (u64)blockIdx.x * KM_TILE;
        if (c) {
            km_lane_close(mask, base, prev1, sa, n, k, min_occ, max_occ, [&](u32 j, u32 row, u32, u32 occ) {
                const u32 ql = (u32)((u64)row + occ - tile_base);
                const u32 pl = row >= tile_base ? (u32)(row - tile_base) : 0xffffu;
                s_stage[before + j] = ql << 16 | pl;
            });
        }
        __syncthreads();
        const u64 o = offs[blockIdx.x];
        for (u32 i = threadIdx.x; i < total; i += KM_NT) {
            const u32 v = s_stage[i];
            const u64 q = tile_base + (v >> 16);
            const u64 p = (v & 0xffffu) == 0xffffu ? (u64)cr - 1u : tile_base + (v & 0xffffu);
            kpos[o + i] = sa[p];
            kocc[o + i] = (u32)(q - p);
            if (krow) krow[o + i] = (u32)p;
        }
    } else {
        __syncthreads();
        for (u32 i = threadIdx.x; i < lds_bins; i += KM_NT) {
            const u32 v = s_hist[i];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(hist + i), (unsigned long long)v);
        }
        if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long *>(distinct), (unsigned long long)total);
    }
}

// The all-k profile: one pass over lcp (each lane 4 rows and one word of halo), two LDS histograms of kmax + 1 bins,
// out[0 .. kmax] += #{r : min(lcp[r], kmax) = i} and out[kmax + 1 .. 2 kmax + 1] the same for min(max(lcp[r], lcp[r + 1]), kmax)
// over the rows 1 .. n.  The saturated bin is counted per wave by ballot and popcount: on periodic or unary text every row
// lands there.  (The other bins take one LDS atomic per row: where the LCP values of a text crowd on a few bins -- iid text,
// around log_sigma n -- those serialise, and the pass runs at 2.6 times a plain read of lcp; naming a bin per wave and adding
// for all lanes that share it, up to four times, was measured and was no faster there and slower elsewhere.)  A workgroup
// takes every gridDim.x-th chunk and flushes once.  sa is not read.
__global__ __launch_bounds__(KM_PF_NT) void km_profile_kernel(const u32 *__restrict__ lcp, u64 N, u32 kmax, u32 aligned,
                                                             u64 *__restrict__ out) {
    __shared__ u32 s_a[KM_MAX_KMAX + 1], s_b[KM_MAX_KMAX + 1];
    for (u32 i = threadIdx.x; i <= kmax; i += KM_PF_NT) { s_a[i] = 0; s_b[i] = 0; }
    __syncthreads();
    u64 sat_a = 0, sat_b = 0;     // wave-uniform
    for (u64 chunk = blockIdx.x; chunk * KM_PF_CHUNK < N; chunk += gridDim.x) {
        const u64 r0 = chunk * KM_PF_CHUNK + (u64)threadIdx.x * KM_PF_ROWS;
        u32 w[KM_PF_ROWS + 1];
        if (aligned && r0 + KM_PF_ROWS <= N) {
            const uint4 x = *reinterpret_cast<const uint4 *>(lcp + r0);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else {
#pragma unroll
            for (u32 i = 0; i < KM_PF_ROWS; i++) w[i] = r0 + i < N ? lcp[r0 + i] : 0u;
        }
        w[KM_PF_ROWS] = r0 + KM_PF_ROWS < N ? lcp[r0 + KM_PF_ROWS] : 0u;
#pragma unroll
        for (u32 i = 0; i < KM_PF_ROWS; i++) {
            const u64 r = r0 + i;
            const bool live = r < N;
            u32 a, b;
            const bool hasb = km_profile_bins(r, N, w[i], w[i + 1], kmax, &a, &b) && live;
            const bool fa = live && a == kmax, fb = hasb && b == kmax;
            sat_a += (u64)__popcll(__ballot(fa));
            sat_b += (u64)__popcll(__ballot(fb));
            if (live && !fa) atomicAdd(&s_a[a], 1u);
            if (hasb && !fb) atomicAdd(&s_b[b], 1u);
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < kmax; i += KM_PF_NT) {
        const u32 va = s_a[i], vb = s_b[i];
        if (va) atomicAdd(reinterpret_cast<unsigned long long *>(out + i), (unsigned long long)va);
        if (vb) atomicAdd(reinterpret_cast<unsigned long long *>(out + kmax + 1u + i), (unsigned long long)vb);
    }
    if (lane_id() == 0) {
        if (sat_a) atomicAdd(reinterpret_cast<unsigned long long *>(out + kmax), (unsigned long long)sat_a);
        if (sat_b) atomicAdd(reinterpret_cast<unsigned long long *>(out + 2u * kmax + 1u), (unsigned long long)sat_b);
    }
}
#endif  // TC_KM_HOST_CHECK
