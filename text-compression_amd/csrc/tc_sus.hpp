// tc_sus.hpp -- what is unique in a text, from its enhanced suffix array: the shortest unique prefix of every suffix, the
// minimal unique substrings (MUS) and the shortest unique substring over every position (included by tc_sus_host.hpp behind
// tc_lz_host.hpp, whose range minimum -- lz_range_min of tc_lz.hpp -- and tc_fm_host.hpp, whose min tree and row search --
// tc_fm_ms.hpp -- it uses unchanged).  No counterpart in the reference.  host/check/sus_kernels.cpp
// compiles sus_prefix_lane, sus_mark_lane, sus_point_lane, the range minimum and the search as plain C++
// (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes); the kernels around the lanes -- tile sums, the two scans -- exist on the
// device only.
//
// include/textcomp.h defines up, a MUS and the point answer.  N = n + 1 rows, sa / lcp as tc_lcp_array defines them.
//   up      one lane per row r: up[sa[r]] = max(lcp[r], lcp[r + 1]) + 1 where that many bytes are left, else 0.  Row 0 is the
//           empty suffix and writes nothing.  sa is a permutation, so every up[i] is written exactly once: no inverse array.
//   MUS     s starts one of length up[s] iff up[s] != 0 and (up[s + 1] = 0 or up[s + 1] >= up[s]), up[n] read as 0: the
//           string without its first byte is a proper prefix of the shortest unique prefix at s + 1, or that suffix has
//           none.  Starts and ends (e = s + up[s] - 1) both increase strictly along the list.
//   point   position-indexed arrays, so nothing depends on the number of MUS and no count crosses to the host:
//             mlen[s]  = up[s] where s starts a MUS, 0xffffffff elsewhere, and a min tree over it (fm_lmin_kernel)
//             pred[p]  = 1 + the start of the MUS with the largest end <= p, 0 if none: endof[e] = s + 1 by a plain store
//                        (ends are distinct) over zeroes, then an inclusive max scan in place (larger end, larger start)
//             nxt[p]   = the smallest MUS start >= p, n if none, nxt[n] = n: a reverse min scan
//           The lane of p: b = pred[p - 1] is the predecessor, s_lo = nxt[b] the first MUS behind it.  Every MUS that starts
//           in [s_lo, p] ends at or behind p (its end is larger than the predecessor's, the largest before p), so these are
//           exactly the covering ones: the shortest is min mlen[s_lo .. p] (lz_range_min), the leftmost of that length s_lo
//           itself or the first entry behind s_lo below m + 1 (fm_ms_next_below).  The successor is nxt[p + 1].  The three
//           candidates go into one u64 each, len << 32 | start, and the smallest wins: by length, then by start.
//           At most 2 f words per tree level for the minimum and for the search, on any text.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
// what host/check/sus_kernels.cpp asserts happened: the answer was [0] a covering MUS, [1] the predecessor extended right,
// [2] the successor extended left; [3] the leftmost minimum was not s_lo (the search ran); [4] no MUS covers p; [5] two
// candidates had one length and the start decided
static u64 sus_seen[6] = {};
#define SUS_SEEN(k) (sus_seen[k]++)
#else
#define SUS_SEEN(k) ((void)0)
#endif

#define SUS_NT 256
#define SUS_ITEMS 8
#define SUS_TILE 2048           // positions per workgroup of the mark, list and scan passes: SUS_NT lanes x SUS_ITEMS in a row
#define SUS_NONE 0xffffffffu
enum { SUS_MARK = 0, SUS_COUNT = 1, SUS_FILL = 2 };

// row r of N: one store of up at sa[r]
FM_MS_DEVICE void sus_prefix_lane(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, u32 N, u32 r, u32 *__restrict__ up) {
    const u32 n = N - 1u, i = sa[r];
    if (i >= n) return;                             // (row 0, the empty suffix; keeps the store inside up on any content)
    const u32 a = lcp[r], b = r + 1u < N ? lcp[r + 1u] : 0u;
    const u32 m = a > b ? a : b;
    up[i] = (u64)i + m < n ? m + 1u : 0u;
}

// u = up[s], v = up[s + 1] (0 for s + 1 = n): does s start a MUS?
FM_MS_DEVICE bool sus_mus_rule(u32 u, u32 v) { return u != 0 && (v == 0 || v >= u); }

// position s < n of the mark pass: mlen[s], and endof at the MUS's end
FM_MS_DEVICE void sus_mark_lane(u32 n, u32 s, u32 u, u32 v, u32 *__restrict__ mlen, u32 *__restrict__ endof) {
    const bool is = sus_mus_rule(u, v);
    mlen[s] = is ? u : SUS_NONE;
    const u64 e = (u64)s + u - 1u;
    if (is && e < n) endof[e] = s + 1u;             // (e < n by the definition of up: keeps the store inside endof)
}

// position p < n: len << 32 | start of its shortest unique substring.  T: the min tree over mlen (T.lcp = mlen, n entries).
FM_MS_DEVICE u64 sus_point_lane(const FmMsTree &T, const u32 *__restrict__ pred, const u32 *__restrict__ nxt, u32 n, u32 p) {
    const u32 *mlen = T.lcp;
    u32 b = p ? pred[p - 1u] : 0u;
    if (b > p) b = 0;                               // (a MUS that ends before p starts before p: b <= p)
    u64 best = ~0ull;
    u32 kind = 3;
    if (b) {
        best = (u64)(p - b + 2u) << 32 | (b - 1u);
        kind = 1;
    }
    const u32 s_lo = nxt[b];
    if (s_lo <= p) {
        const u32 m = lz_range_min<4>(T, s_lo, p);
        u32 s = s_lo;
        if (mlen[s_lo] != m) {
            SUS_SEEN(3);
            s = fm_ms_next_below(T, n, s_lo, m + 1u);
        }
        const u64 c = (u64)m << 32 | s;
        if ((c >> 32) == (best >> 32)) SUS_SEEN(5);
        if (c < best) {
            best = c;
            kind = 0;
        }
    } else {
        SUS_SEEN(4);
    }
    const u32 s2 = nxt[p + 1u];
    if (s2 < n) {
        const u64 c = (u64)(s2 - p + mlen[s2]) << 32 | p;
        if ((c >> 32) == (best >> 32)) SUS_SEEN(5);
        if (c < best) {
            best = c;
            kind = 2;
        }
    }
    if (kind < 3) SUS_SEEN(kind);
    return best;
}

#ifndef TC_FM_MS_HOST_CHECK
// One lane per row: coalesced reads of sa and lcp, one scattered 4-byte store.
FM_MS_SMALL_KERNEL sus_prefix_kernel(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, u32 N, u32 *__restrict__ up) {
    const u64 r = (u64)blockIdx.x * FM_MS_NT + threadIdx.x;
    if (r < N) sus_prefix_lane(sa, lcp, N, (u32)r, up);
}

// A tile of SUS_TILE positions per workgroup, SUS_ITEMS positions in a row per lane (and the one behind them).
//   SUS_MARK   mlen and endof (zeroed before) of every position, no filter
//   SUS_COUNT  tilecnt[t] = the MUS of the tile with min_len <= len (<= max_len unless that is 0)
//   SUS_FILL   the same MUS again, in start order from slot offs[t] on; nothing at or behind slot `total` is written
template <int MODE>
__global__ __launch_bounds__(SUS_NT) void sus_mark_kernel(const u32 *__restrict__ up, u32 n, u32 min_len, u32 max_len,
                                                          u32 *__restrict__ mlen, u32 *__restrict__ endof, u64 *__restrict__ tilecnt,
                                                          const u64 *__restrict__ offs, u64 total, u32 *__restrict__ mus_start,
                                                          u32 *__restrict__ mus_len) {
    __shared__ u32 s_scan[SUS_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * SUS_TILE + (u64)threadIdx.x * SUS_ITEMS;
    u32 u[SUS_ITEMS + 1];
#pragma unroll
    for (u32 k = 0; k <= SUS_ITEMS; k++) u[k] = base + k < n ? up[base + k] : 0u;
    u32 c = 0, pass = 0;
#pragma unroll
    for (u32 k = 0; k < SUS_ITEMS; k++) {
        if (base + k >= n) break;
        if (MODE == SUS_MARK) {
            sus_mark_lane(n, (u32)(base + k), u[k], u[k + 1], mlen, endof);
        } else if (sus_mus_rule(u[k], u[k + 1]) && u[k] >= min_len && (max_len == 0 || u[k] <= max_len)) {
            pass |= 1u << k;
            c++;
        }
    }
    if (MODE == SUS_MARK) return;
    u32 tile_total;
    const u32 before = block_excl_sum<SUS_NT>(c, s_scan, &tile_total);
    if (MODE == SUS_COUNT) {
        if (threadIdx.x == 0) tilecnt[blockIdx.x] = tile_total;
        return;
    }
    u64 slot = offs[blockIdx.x] + before;
#pragma unroll
    for (u32 k = 0; k < SUS_ITEMS; k++) {
        if (!(pass >> k & 1u) || slot >= total) continue;
        mus_start[slot] = (u32)(base + k);
        mus_len[slot] = u[k];
        slot++;
    }
}

// The two scans of the point call, as tc_scan64 runs its sums: per tile, a spine, per tile again.
// tmax[t] = the largest endof of tile t, tmin[t] = its smallest MUS start (n if it has none)
__global__ __launch_bounds__(SUS_NT) void sus_reduce_kernel(const u32 *__restrict__ endof, const u32 *__restrict__ mlen, u32 n,
                                                            u32 *__restrict__ tmax, u32 *__restrict__ tmin) {
    __shared__ u32 s_max[SUS_NT / 64], s_min[SUS_NT / 64];
    const u64 base = (u64)blockIdx.x * SUS_TILE;
    u32 hi = 0, lo = n;
#pragma unroll
    for (u32 k = 0; k < SUS_ITEMS; k++) {
        const u64 i = base + k * SUS_NT + threadIdx.x;
        if (i >= n) continue;
        const u32 e = endof[i];
        hi = e > hi ? e : hi;
        if (mlen[i] != SUS_NONE && (u32)i < lo) lo = (u32)i;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 a = __shfl_xor(hi, d, 64), b = __shfl_xor(lo, d, 64);
        hi = a > hi ? a : hi;
        lo = b < lo ? b : lo;
    }
    if ((threadIdx.x & 63) == 0) {
        s_max[threadIdx.x >> 6] = hi;
        s_min[threadIdx.x >> 6] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 w = 1; w < SUS_NT / 64; w++) {
            hi = s_max[w] > hi ? s_max[w] : hi;
            lo = s_min[w] < lo ? s_min[w] : lo;
        }
        tmax[blockIdx.x] = hi;
        tmin[blockIdx.x] = lo;
    }
}
// single workgroup, in place: tmax[t] = the maximum over the tiles before t (0), tmin[t] = the minimum over those behind t (n)
__global__ __launch_bounds__(1024) void sus_spine_kernel(u32 *tmax, u32 *tmin, u32 tiles, u32 n) {
    __shared__ u32 s_max[1024], s_min[1024];
    const u32 per = (tiles + 1023u) / 1024u;
    const u32 lo = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
    u32 a = 0, b = n;
    for (u32 t = lo; t < hi; t++) {
        a = tmax[t] > a ? tmax[t] : a;
        b = tmin[t] < b ? tmin[t] : b;
    }
    s_max[threadIdx.x] = a;
    s_min[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int i = 0; i < 1024; i++) {
            const u32 c = s_max[i];
            s_max[i] = run;
            run = c > run ? c : run;
        }
        run = n;
        for (int i = 1023; i >= 0; i--) {
            const u32 c = s_min[i];
            s_min[i] = run;
            run = c < run ? c : run;
        }
    }
    __syncthreads();
    u32 run = s_max[threadIdx.x];
    for (u32 t = lo; t < hi; t++) {
        const u32 c = tmax[t];
        tmax[t] = run;
        run = c > run ? c : run;
    }
    run = s_min[threadIdx.x];
    for (u32 t = hi; t > lo; t--) {
        const u32 c = tmin[t - 1u];
        tmin[t - 1u] = run;
        run = c < run ? c : run;
    }
}
// pred[p] = the maximum of endof[0 .. p], in place over endof (a lane reads its own entries before it writes them);
// nxt[p] = the smallest MUS start >= p or n, nxt[n] = n
__global__ __launch_bounds__(SUS_NT) void sus_scan_kernel(u32 *pred, const u32 *__restrict__ mlen, u32 n, const u32 *__restrict__ tmax,
                                                          const u32 *__restrict__ tmin, u32 *__restrict__ nxt) {
    __shared__ u32 s_max[SUS_NT / 64], s_min[SUS_NT / 64];
    const u64 base = (u64)blockIdx.x * SUS_TILE + (u64)threadIdx.x * SUS_ITEMS;
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    u32 e[SUS_ITEMS], st[SUS_ITEMS], hi = 0, lo = n;
#pragma unroll
    for (u32 k = 0; k < SUS_ITEMS; k++) {
        const u64 i = base + k;
        e[k] = i < n ? pred[i] : 0u;
        st[k] = i < n && mlen[i] != SUS_NONE ? (u32)i : n;
        hi = e[k] > hi ? e[k] : hi;
        lo = st[k] < lo ? st[k] : lo;
    }
    u32 imax = hi, imin = lo;       // inclusive over the wave: the maximum up to this lane, the minimum from it on
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 a = __shfl_up(imax, d, 64), b = __shfl_down(imin, d, 64);
        if ((int)lane >= d) imax = a > imax ? a : imax;
        if ((int)lane + d < 64) imin = b < imin ? b : imin;
    }
    if (lane == 63) s_max[w] = imax;
    if (lane == 0) s_min[w] = imin;
    u32 run_max = __shfl_up(imax, 1, 64), run_min = __shfl_down(imin, 1, 64);
    if (lane == 0) run_max = 0;
    if (lane == 63) run_min = n;
    __syncthreads();
    const u32 t0 = tmax[blockIdx.x], t1 = tmin[blockIdx.x];
    run_max = t0 > run_max ? t0 : run_max;
    run_min = t1 < run_min ? t1 : run_min;
#pragma unroll
    for (u32 i = 0; i < SUS_NT / 64; i++) {
        if (i < w) run_max = s_max[i] > run_max ? s_max[i] : run_max;
        if (i > w) run_min = s_min[i] < run_min ? s_min[i] : run_min;
    }
#pragma unroll
    for (u32 k = 0; k < SUS_ITEMS; k++) {
        run_max = e[k] > run_max ? e[k] : run_max;
        if (base + k < n) pred[base + k] = run_max;
    }
#pragma unroll
    for (u32 k = SUS_ITEMS; k-- > 0;) {
        run_min = st[k] < run_min ? st[k] : run_min;
        if (base + k < n) nxt[base + k] = run_min;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) nxt[n] = n;
}

// One lane per position.  sus_start may be null.
FM_MS_KERNEL sus_point_kernel(const u32 *__restrict__ mlen, const u32 *__restrict__ lmin, const u32 *__restrict__ pred,
                              const u32 *__restrict__ nxt, u32 n, u32 lf, u32 *__restrict__ sus_start, u32 *__restrict__ sus_len) {
    __shared__ u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    if (threadIdx.x == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(n, lf, s_off, s_cnt, &words);
    }
    __syncthreads();
    const u64 p = (u64)blockIdx.x * FM_MS_NT + threadIdx.x;
    if (p >= n) return;
    FmMsTree T;
    T.lcp = mlen; T.lmin = lmin; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    const u64 best = sus_point_lane(T, pred, nxt, n, (u32)p);
    if (sus_start) sus_start[p] = (u32)best;
    sus_len[p] = (u32)(best >> 32);
}
#endif  // TC_FM_MS_HOST_CHECK
