// tc_cov.hpp -- the repeat cover of a text: which bytes lie in repeated content, as spans, as a mask and as the text without
// them (included by tc_cov_host.hpp behind tc_sus_host.hpp; it uses the min tree and the row searches of tc_fm_ms.hpp and the
// range minimum of tc_lz.hpp unchanged).  No counterpart in the reference.
// host/check/cover_kernels.cpp compiles cov_seed_kernel, cov_reach and cov_lane_bits as plain C++ (TC_FM_MS_HOST_CHECK, as
// tc_fm_ms.hpp describes); the kernels around the lanes -- tile maxima, the spine, the LDS scans, the compaction -- exist on the
// device only.
//
// include/textcomp.h defines a seed, the cover, the spans, the mask and the dedup.  N = n + 1 rows, sa / lcp as tc_lcp_array
// defines them, L = min_len, q = min_occ.
//   seeds   one lane per row r, i = sa[r].  The row leaves at once if i + L > n or max(lcp[r], lcp[r + 1]) < L: its L-mer occurs
//           once.  For ALL and q = 2 that is the answer.  Otherwise the L-mer's rows are [lo, hi), lo = the nearest row at or
//           above r with lcp < L (fm_ms_prev_below), hi = the nearest row below r with lcp < L (fm_ms_next_below), and
//           occ = hi - lo.  For LATER i must not be the minimum of sa[lo .. hi): one lz_range_min over the min tree of sa.  A seed
//           stores len[i] = L into an array of zeroes: one scattered 4-byte store, non-seeds store nothing, sa is a permutation
//           so no entry is written twice.  At most 2 f words per tree level and search on any text; no lane walks over rows.
//   cover   over ANY array len of n words: reach[i] = min(n, i + len[i]) where len[i] >= L, else 0 (the sum in 64 bits: a value
//           is compared and added, never used as an index), M[p] = the maximum of reach[0 .. p], and p is covered iff M[p] > p.
//           M is a max scan over tiles of COV_TILE positions, as sus_scan_kernel runs its scans: cov_reduce_kernel takes the
//           tiles' maxima, cov_spine_kernel turns them into the exclusive prefix maximum in one workgroup, and every later pass
//           redoes its tile's scan in registers and LDS from that carry.  A reach that crosses tiles without a seed arrives by
//           the carry; no lane walks along a span.
//   spans   p starts one iff it is covered and p - 1 is not; p ends one iff it is covered and p + 1 is not, which needs the
//           one element behind the lane's positions (as sus_mark_kernel reads it).  cov_count_kernel: starts and covered bytes
//           per tile; tc_scan64 over both; cov_fill_kernel writes the k-th start to span_start[k] and the k-th end + 1 to
//           span_len[k] -- the starts at or before p give the rank of an end at p -- and cov_len_kernel subtracts.  No atomics;
//           the order is the text's.
//   mask    cov_mask_kernel: one pass over 8 bytes per lane, the 256-byte map in LDS (it arrives as a kernel argument).
//   dedup   the kept bytes before tile t are t COV_TILE - (the covered bytes before it).  cov_dedup_kernel compacts the tile's
//           kept bytes in LDS and stores them as one run: a few head bytes, aligned 4-byte words, a few tail bytes.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
// what host/check/cover_kernels.cpp asserts happened: [0] a reach was clamped to n, [1] a group of exactly q rows, [2] a group
// of q - 1 rows, [3] a leftmost occurrence refused under LATER, [4] the row test alone answered (ALL, q = 2)
static u64 cov_seen[5] = {};
#define COV_SEEN(k) (cov_seen[k]++)
#else
#define COV_SEEN(k) ((void)0)
#endif

#define COV_NT 256
#define COV_ITEMS 8
#define COV_TILE 2048           // positions per workgroup of every pass: COV_NT lanes x COV_ITEMS in a row per lane, as SUS_TILE

// row r of N: len[sa[r]] = L where sa[r] is a seed.  T: the min tree of lcp, S: that of sa (one shape); neither is read for
// ALL with q = 2, S only for LATER.
template <bool LATER>
FM_MS_DEVICE void cov_seed_lane(const FmMsTree &T, const FmMsTree &S, u32 N, u32 r, u32 L, u32 q, u32 *__restrict__ len) {
    const u32 n = N - 1u, i = S.lcp[r];             // (level 0 of S is sa)
    if ((u64)i + L > n) return;                     // (row 0, the empty suffix, leaves here: L >= 1; keeps the store inside len)
    const u32 a = T.lcp[r], b = r + 1u < N ? T.lcp[r + 1u] : 0u;
    if ((a > b ? a : b) < L) return;
    if (!LATER && q == 2) {
        COV_SEEN(4);
        len[i] = L;
        return;
    }
    const u32 lo = fm_ms_prev_below(T, r, L), hi = fm_ms_next_below(T, N, r, L);
    if (hi - lo == q) COV_SEEN(1);
    if (hi - lo + 1u == q) COV_SEEN(2);
    if (hi <= lo || hi - lo < q) return;
    if (LATER && lz_range_min<5>(S, lo, hi - 1u) >= i) {
        COV_SEEN(3);
        return;
    }
    len[i] = L;
}

// One lane per row: coalesced reads of sa and lcp, the searches, one scattered 4-byte store.
template <bool LATER>
FM_MS_KERNEL cov_seed_kernel(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, const u32 *__restrict__ sa_min,
                             const u32 *__restrict__ lcp_min, u32 N, u32 lf, u32 L, u32 q, u32 *__restrict__ len) {
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 r = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (r >= N) return;
    FmMsTree T, S;
    T.lcp = lcp; T.lmin = lcp_min; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    S = T;
    S.lcp = sa; S.lmin = sa_min;
    cov_seed_lane<LATER>(T, S, N, (u32)r, L, q, len);
}

// where position i stops counting: min(n, i + l) for l >= L, 0 for a position that does not count
FM_MS_DEVICE u32 cov_reach(u32 n, u64 i, u32 l, u32 L) {
    if (l < L) return 0;
    const u64 e = i + l;
    if (e > n) COV_SEEN(0);
    return e < n ? (u32)e : n;
}

// The lane of the positions base .. base + COV_ITEMS - 1 (those below n).  r: their reaches and the reach of the one position
// behind them (0 where that is n or more); run: the maximum of every reach before base.  Bit k of cov: base + k is covered;
// of st: it starts a span; of en: it ends one.
struct CovBits {
    u32 cov, st, en;
};
FM_MS_DEVICE CovBits cov_lane_bits(u32 n, u64 base, const u32 *r, u32 run) {
    CovBits b = {0, 0, 0};
    bool prev = base != 0 && run >= base;           // M[base - 1] > base - 1
    u32 m = run;
    for (u32 k = 0; k < COV_ITEMS; k++) {
        const u64 p = base + k;
        if (p >= n) break;
        m = r[k] > m ? r[k] : m;
        const bool c = m > p;
        const bool next = p + 1 < n && (r[k + 1] > m ? r[k + 1] : m) > p + 1;
        if (c) b.cov |= 1u << k;
        if (c && !prev) b.st |= 1u << k;
        if (c && !next) b.en |= 1u << k;
        prev = c;
    }
    return b;
}

#ifndef TC_FM_MS_HOST_CHECK
// the 256-byte map of the mask, as a kernel argument
struct CovMap {
    u32 w[64];
};

// tmax[t] = the largest reach of tile t
__global__ __launch_bounds__(COV_NT) void cov_reduce_kernel(const u32 *__restrict__ len, u32 n, u32 L, u32 *__restrict__ tmax) {
    __shared__ u32 s_max[COV_NT / 64];
    const u64 base = (u64)blockIdx.x * COV_TILE;
    u32 hi = 0;
#pragma unroll
    for (u32 k = 0; k < COV_ITEMS; k++) {
        const u64 i = base + k * COV_NT + threadIdx.x;
        if (i >= n) continue;
        const u32 e = cov_reach(n, i, len[i], L);
        hi = e > hi ? e : hi;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 a = __shfl_xor(hi, d, 64);
        hi = a > hi ? a : hi;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 w = 1; w < COV_NT / 64; w++) hi = s_max[w] > hi ? s_max[w] : hi;
        tmax[blockIdx.x] = hi;
    }
}
// single workgroup, in place: tmax[t] = the maximum over the tiles before t (0 for t = 0)
__global__ __launch_bounds__(1024) void cov_spine_kernel(u32 *tmax, u32 tiles) {
    __shared__ u32 s_max[1024];
    const u32 per = (tiles + 1023u) / 1024u;
    const u32 lo = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
    u32 a = 0;
    for (u32 t = lo; t < hi; t++) a = tmax[t] > a ? tmax[t] : a;
    s_max[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int i = 0; i < 1024; i++) {
            const u32 c = s_max[i];
            s_max[i] = run;
            run = c > run ? c : run;
        }
    }
    __syncthreads();
    u32 run = s_max[threadIdx.x];
    for (u32 t = lo; t < hi; t++) {
        const u32 c = tmax[t];
        tmax[t] = run;
        run = c > run ? c : run;
    }
}

// The tile of this workgroup: the lane's reaches (and the one behind them) into r, and what every later pass starts from -- the
// maximum of every reach before the lane's first position, the carry of the tiles before included.  s_max: COV_NT / 64 words.
__device__ __forceinline__ u32 cov_tile_run(const u32 *__restrict__ len, u32 n, u32 L, u64 base, u32 carry, u32 (&r)[COV_ITEMS + 1],
                                            u32 *s_max) {
    u32 l[COV_ITEMS + 1];
    if (base + COV_ITEMS < n && (reinterpret_cast<uintptr_t>(len) & 15u) == 0) {    // (base is a multiple of 8 words)
        const uint4 a = *reinterpret_cast<const uint4 *>(len + base), b = *reinterpret_cast<const uint4 *>(len + base + 4);
        l[0] = a.x; l[1] = a.y; l[2] = a.z; l[3] = a.w;
        l[4] = b.x; l[5] = b.y; l[6] = b.z; l[7] = b.w;
        l[8] = len[base + 8];
    } else {
#pragma unroll
        for (u32 k = 0; k <= COV_ITEMS; k++) l[k] = base + k < n ? len[base + k] : 0u;
    }
    u32 hi = 0;
#pragma unroll
    for (u32 k = 0; k <= COV_ITEMS; k++) {
        r[k] = base + k < n ? cov_reach(n, base + k, l[k], L) : 0u;
        if (k < COV_ITEMS) hi = r[k] > hi ? r[k] : hi;
    }
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const u32 imax = wave_incl_max(hi);
    if (lane == 63) s_max[w] = imax;
    u32 run = __shfl_up(imax, 1, 64);
    if (lane == 0) run = 0;
    __syncthreads();
    run = carry > run ? carry : run;
#pragma unroll
    for (u32 i = 0; i < COV_NT / 64; i++)
        if (i < w) run = s_max[i] > run ? s_max[i] : run;
    return run;
}

// cnt_s[t] = the spans that start in tile t, cnt_c[t] = its covered bytes
__global__ __launch_bounds__(COV_NT) void cov_count_kernel(const u32 *__restrict__ len, u32 n, u32 L, const u32 *__restrict__ tmax,
                                                           u64 *__restrict__ cnt_s, u64 *__restrict__ cnt_c) {
    __shared__ u32 s_max[COV_NT / 64], s_scan[COV_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * COV_TILE + (u64)threadIdx.x * COV_ITEMS;
    u32 r[COV_ITEMS + 1];
    const u32 run = cov_tile_run(len, n, L, base, tmax[blockIdx.x], r, s_max);
    const CovBits b = cov_lane_bits(n, base, r, run);
    u32 total;      // (both sums in one word: at most COV_TILE covered bytes, at most COV_TILE / 2 starts)
    block_excl_sum<COV_NT>((u32)__popc(b.st) << 16 | (u32)__popc(b.cov), s_scan, &total);
    if (threadIdx.x == 0) {
        cnt_s[blockIdx.x] = total >> 16;
        cnt_c[blockIdx.x] = total & 0xffffu;
    }
}

// span_start[k] = the k-th start, span_end[k] = the k-th end + 1, k counted from offs_s[t] on; nothing at or behind slot
// `total` is written
__global__ __launch_bounds__(COV_NT) void cov_fill_kernel(const u32 *__restrict__ len, u32 n, u32 L, const u32 *__restrict__ tmax,
                                                          const u64 *__restrict__ offs_s, u64 total, u32 *__restrict__ span_start,
                                                          u32 *__restrict__ span_end) {
    __shared__ u32 s_max[COV_NT / 64], s_scan[COV_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * COV_TILE + (u64)threadIdx.x * COV_ITEMS;
    u32 r[COV_ITEMS + 1];
    const u32 run = cov_tile_run(len, n, L, base, tmax[blockIdx.x], r, s_max);
    const CovBits b = cov_lane_bits(n, base, r, run);
    u32 tile_total;
    const u32 before = block_excl_sum<COV_NT>((u32)__popc(b.st), s_scan, &tile_total);
    u64 slot = offs_s[blockIdx.x] + before;     // the starts before the lane's first position
#pragma unroll
    for (u32 k = 0; k < COV_ITEMS; k++) {
        if (b.st >> k & 1u) {
            if (slot < total) span_start[slot] = (u32)(base + k);
            slot++;
        }
        if ((b.en >> k & 1u) && slot != 0 && slot - 1 < total) span_end[slot - 1] = (u32)(base + k + 1);
    }
}
// span_len[k] = end + 1 - start
__global__ __launch_bounds__(256) void cov_len_kernel(const u32 *__restrict__ span_start, u32 *__restrict__ span_len, u64 total) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < total) span_len[k] -= span_start[k];
}

// the lane's COV_ITEMS text bytes from base on, byte k in bits 8 k (zeroes behind the text)
__device__ __forceinline__ u64 cov_load_bytes(const u8 *__restrict__ text, u32 n, u64 base) {
    if (base + COV_ITEMS <= n && (reinterpret_cast<uintptr_t>(text) & 7u) == 0) return *reinterpret_cast<const u64 *>(text + base);
    u64 v = 0;
#pragma unroll
    for (u32 k = 0; k < COV_ITEMS; k++)
        if (base + k < n) v |= (u64)text[base + k] << (8 * k);
    return v;
}

// out[p] = map[text[p]] where p is covered and text[p] elsewhere; without a map (has_map = 0; text is not read) 1 and 0
__global__ __launch_bounds__(COV_NT) void cov_mask_kernel(const u32 *__restrict__ len, u32 n, u32 L, const u32 *__restrict__ tmax,
                                                          const u8 *__restrict__ text, CovMap map, u32 has_map, u8 *__restrict__ out) {
    __shared__ u32 s_max[COV_NT / 64], s_map[64];
    if (threadIdx.x < 64) s_map[threadIdx.x] = map.w[threadIdx.x];
    const u64 base = (u64)blockIdx.x * COV_TILE + (u64)threadIdx.x * COV_ITEMS;
    u32 r[COV_ITEMS + 1];
    const u32 run = cov_tile_run(len, n, L, base, tmax[blockIdx.x], r, s_max);      // (its barrier also publishes s_map)
    const CovBits b = cov_lane_bits(n, base, r, run);
    if (base >= n) return;
    const u64 in = has_map ? cov_load_bytes(text, n, base) : 0ull;
    const u8 *const m8 = reinterpret_cast<const u8 *>(s_map);
    u64 v = 0;
#pragma unroll
    for (u32 k = 0; k < COV_ITEMS; k++) {
        const u32 c = b.cov >> k & 1u, x = (u32)(in >> (8 * k)) & 255u;
        v |= (u64)(has_map ? (c ? (u32)m8[x] : x) : c) << (8 * k);
    }
    if (base + COV_ITEMS <= n && (reinterpret_cast<uintptr_t>(out) & 7u) == 0) {
        *reinterpret_cast<u64 *>(out + base) = v;
    } else {
#pragma unroll
        for (u32 k = 0; k < COV_ITEMS; k++)
            if (base + k < n) out[base + k] = (u8)(v >> (8 * k));
    }
}

// kept[t] = the uncovered bytes of tile t, in order, stored from out[t COV_TILE - offs_c[t]] on; nothing at or behind out[limit]
// is written
__global__ __launch_bounds__(COV_NT) void cov_dedup_kernel(const u32 *__restrict__ len, u32 n, u32 L, const u32 *__restrict__ tmax,
                                                           const u8 *__restrict__ text, const u64 *__restrict__ offs_c, u64 limit,
                                                           u8 *__restrict__ out) {
    __shared__ u32 s_max[COV_NT / 64], s_scan[COV_NT / 64 + 1];
    __shared__ __attribute__((aligned(16))) u8 s_buf[COV_TILE];
    const u64 tile0 = (u64)blockIdx.x * COV_TILE, base = tile0 + (u64)threadIdx.x * COV_ITEMS;
    u32 r[COV_ITEMS + 1];
    const u32 run = cov_tile_run(len, n, L, base, tmax[blockIdx.x], r, s_max);
    const CovBits b = cov_lane_bits(n, base, r, run);
    const u32 valid = base >= n ? 0u : (n - base < COV_ITEMS ? (u32)(n - base) : (u32)COV_ITEMS);
    const u32 keep = ~b.cov & ((1u << valid) - 1u);
    u32 kept;
    u32 at = block_excl_sum<COV_NT>((u32)__popc(keep), s_scan, &kept);
    const u64 in = keep ? cov_load_bytes(text, n, base) : 0ull;
#pragma unroll
    for (u32 k = 0; k < COV_ITEMS; k++)
        if (keep >> k & 1u) s_buf[at++] = (u8)(in >> (8 * k));
    __syncthreads();
    const u64 covered_before = offs_c[blockIdx.x];
    const u64 dst = covered_before <= tile0 ? tile0 - covered_before : limit;
    if (dst >= limit) return;
    if (kept > limit - dst) kept = (u32)(limit - dst);
    u8 *const o = out + dst;
    u32 head = (4u - (u32)(reinterpret_cast<uintptr_t>(o) & 3u)) & 3u;
    head = head < kept ? head : kept;
    const u32 words = (kept - head) >> 2, tail = head + 4u * words;
    if (threadIdx.x < head) o[threadIdx.x] = s_buf[threadIdx.x];
    for (u32 j = threadIdx.x; j < words; j += COV_NT) {
        const u32 s = head + 4u * j;
        *reinterpret_cast<u32 *>(o + s) = (u32)s_buf[s] | (u32)s_buf[s + 1] << 8 | (u32)s_buf[s + 2] << 16 | (u32)s_buf[s + 3] << 24;
    }
    if (threadIdx.x < kept - tail) o[tail + threadIdx.x] = s_buf[tail + threadIdx.x];
}
#endif  // TC_FM_MS_HOST_CHECK
