// tc_tm.hpp -- one text held against another: the matching statistics of a query Q (a bytes) against a target T (b bytes),
// their maximal exact matches and their longest common substring (included by tc_tm_host.hpp behind tc_lz_host.hpp, whose
// range minimum -- tc_lz.hpp -- and row searches -- tc_fm_ms.hpp -- it uses unchanged).  No
// counterpart in the reference.  host/check/tm_kernels.cpp compiles tm_row_kernel as plain C++ (TC_FM_MS_HOST_CHECK, as
// tc_fm_ms.hpp describes); the flag, compaction and MEM kernels are streaming passes and exist on the device only.
//
// ms_len[i] = the largest l such that Q[i .. i + l) occurs in T, ms_pos[i] = the start in T of the smallest suffix of T
// that has that string as a prefix, ms_occ[i] = its occurrences in T (include/textcomp.h has the definitions in full).
//
// The enhanced suffix array of X = Q T, n = a + b, N = n + 1 rows, without a separator: both texts may hold all 256 byte
// values, so no byte is free to be one.  A T ROW is a row with a <= sa[r] < n, a Q ROW one with sa[r] < a; row 0 (sa = n)
// is neither.  Three facts make the concatenation enough:
//   i    T's suffixes in X are T's own suffixes and end where X ends, so their order in sa is T's own suffix-array order,
//        and a common prefix with a T row is a true match inside T;
//   ii   for a Q row r, i = sa[r], the longest match of X[i ..) with any T suffix is attained at the nearest T row above
//        r (p) or below r (q): m = max(min lcp[p + 1 .. r], min lcp[r + 1 .. q]).  That match may run over Q's end into
//        T's head; min(., a - i) is monotone, so ms_len[i] = min(m, a - i).  THE CLAMP is the one place where the
//        concatenation shows: "ab" against "abab" has m = 4 at i = 0;
//   iii  with l = ms_len[i] >= 1 the rows whose suffix shares l bytes with row r are the interval [lo, hi], lo = the
//        largest row <= r with lcp < l, hi + 1 = the smallest row > r with lcp < l, or N.  The T rows in it are exactly
//        the occurrences in T (the Q rows in it do not count), and there is one: the neighbour that attained m.
// Two arrays answer every "nearest T row" and every count without a search: cnt[r] = the number of T rows below r, r in
// 0 .. N (an exclusive scan of the flags, tc_scan64), and trow[k] = the k-th T row (a compaction behind that scan).  So
//   p = trow[cnt[r] - 1], q = trow[cnt[r]], ms_occ = cnt[hi + 1] - cnt[lo], ms_pos = sa[trow[cnt[lo]]] - a.
// The same compaction writes qrow[k] = the k-th Q row (row r >= 1 has r - 1 - cnt[r] Q rows below it): the row kernel is
// launched over the a entries of qrow, one lane per Q row, and its cost does not grow with b.  A lane does two reads of
// trow, two range minima and -- where positions or counts are asked for -- the two row searches at depth l: at most
// 2 f words per tree level and search on any text; it walks neither rows nor text.
//
// The three results are stored at position i straight from the row kernel, 4 bytes each, scattered as sa is.  A packed
// word as in lz_lpf_kernel would be 16 bytes per position here (three words, ms_pos and ms_occ each optional) with a pass
// to unpack it: 16 a bytes more scratch and 28 a bytes more traffic to save two of three scattered lines per lane.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
static u64 tm_clamped = 0;                      // positions whose match ran over Q's end
#define TM_CLAMPED() (tm_clamped++)
#else
#define TM_CLAMPED() ((void)0)
#endif

#define TM_NT 256
#define TM_ITEMS 4
#define TM_TILE (TM_NT * TM_ITEMS)              // positions per tile of the MEM count and fill passes
#define TM_ALL 0xffffffffu                      // tm_row_kernel's `only`: every position

// One lane per Q row.  lmin: the min tree (fm_lmin_kernel, fan-out 2^lf) over lcp; cnt: N + 1 entries; trow: b >= 1
// entries; qrow: a entries.  POS = false writes ms_len alone (no search); POS = true also ms_pos and ms_occ, each where it
// is not null.  only = TM_ALL: every position, results stored at index i; only = a position: that position alone, its
// results stored at index 0 (the other lanes leave after their two reads: what tc_text_lcs asks of the one position it
// reports).  The guards hold on an enhanced suffix array; they keep every index in bounds on anything else.
template <bool POS>
FM_MS_KERNEL tm_row_kernel(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, const u32 *__restrict__ lmin, u32 N, u32 lf,
                           const u64 *__restrict__ cnt, const u32 *__restrict__ trow, const u32 *__restrict__ qrow, u32 a, u32 b,
                           u32 only, u32 *__restrict__ ms_len, u32 *__restrict__ ms_pos, u32 *__restrict__ ms_occ) {
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 k = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (k >= a) return;
    const u32 r = qrow[k];
    if (r == 0 || r >= N) return;
    const u32 i = sa[r];
    if (i >= a || (only != TM_ALL && i != only)) return;
    const u32 at = only != TM_ALL ? 0u : i;
    FmMsTree T;
    T.lcp = lcp; T.lmin = lmin; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    const u32 c = (u32)cnt[r];                  // the T rows above r
    u32 m = 0;
    if (c >= 1 && c <= b) {
        const u32 p = trow[c - 1u];
        if (p < r) m = lz_range_min<1>(T, p + 1u, r);
    }
    if (c < b) {
        const u32 q = trow[c];
        if (q > r && q < N) {
            const u32 mq = lz_range_min<1>(T, r + 1u, q);
            m = mq > m ? mq : m;
        }
    }
    u32 l = m;
    if (a - i < m) {                            // the match runs over Q's end into T's head
        l = a - i;
        TM_CLAMPED();
    }
    ms_len[at] = l;
    if (!POS) return;
    u32 pos = 0, occ = 0;
    if (l) {                                    // (the searches need d >= 1)
        const u32 lo = fm_ms_prev_below(T, r, l);
        const u32 hi1 = fm_ms_next_below(T, N, r, l);       // hi + 1 <= N
        const u32 clo = (u32)cnt[lo], chi = (u32)cnt[hi1 < N ? hi1 : N];
        const u32 first = trow[clo < b ? clo : b - 1u];     // the first T row of [lo, hi]
        occ = chi - clo;
        pos = sa[first < N ? first : 0u] - a;
    }
    if (ms_pos) ms_pos[at] = pos;
    if (ms_occ) ms_occ[at] = occ;
}

#ifndef TC_FM_MS_HOST_CHECK
// flag[r] = 1 for a T row, r in 0 .. N (flag[N] = 0: the scan over N + 1 entries leaves cnt[N] = b)
__global__ __launch_bounds__(256) void tm_flag_kernel(const u32 *__restrict__ sa, u32 N, u32 a, u32 n, u64 *__restrict__ flag) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r > N) return;
    u32 f = 0;
    if (r < N) {
        const u32 s = sa[r];
        f = s >= a && s < n ? 1u : 0u;
    }
    flag[r] = f;
}

// trow[k] = the k-th T row, qrow[k] = the k-th Q row, in row order: one lane per row r >= 1, its slot from cnt[r]
__global__ __launch_bounds__(256) void tm_compact_kernel(const u32 *__restrict__ sa, u32 N, u32 a, u32 n, const u64 *__restrict__ cnt,
                                                         u32 *__restrict__ trow, u32 *__restrict__ qrow) {
    const u64 r64 = (u64)blockIdx.x * 256 + threadIdx.x + 1u;
    if (r64 >= N) return;
    const u32 r = (u32)r64, s = sa[r], c = (u32)cnt[r], b = n - a;
    if (s >= a && s < n) {
        if (c < b) trow[c] = r;
    } else if (s < a) {
        const u32 k = r - 1u - c;
        if (c < r && k < a) qrow[k] = r;
    }
}

// ---- maximal exact matches: the positions i with ms_len[i] >= min_len whose match is not the tail of the match one
// position to the left (i = 0 or ms_len[i - 1] <= ms_len[i]): the rule of tc_fm_mems.  The array values are only compared
// and copied, so the two passes stay in bounds on any contents.
__device__ __forceinline__ bool tm_mem_is(u32 prev, u32 l, u64 i, u32 min_len) { return l >= min_len && (i == 0 || prev <= l); }

// cnt[t] = the MEMs that start in tile t
__global__ __launch_bounds__(TM_NT) void tm_mem_count_kernel(const u32 *__restrict__ ms_len, u64 a, u32 min_len, u64 *__restrict__ cnt) {
    __shared__ u32 s[TM_NT / 64];
    const u64 base = (u64)blockIdx.x * TM_TILE;
    u32 c = 0;
    for (u32 k = 0; k < TM_ITEMS; k++) {
        const u64 i = base + (u64)k * TM_NT + threadIdx.x;
        if (i < a) c += tm_mem_is(i ? ms_len[i - 1] : 0u, ms_len[i], i, min_len) ? 1u : 0u;
    }
    c = wave_sum(c);
    if (lane_id() == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 tot = 0;
        for (u32 w = 0; w < TM_NT / 64; w++) tot += s[w];
        cnt[blockIdx.x] = tot;
    }
}

// the MEMs of tile t to the three arrays from slot offs[t] on, in increasing i: lane k owns the positions
// [k TM_ITEMS, k TM_ITEMS + TM_ITEMS) of the tile (and reads the one before them: the halo), a workgroup scan gives its
// first slot.  No slot at or above `slots` is written.
__global__ __launch_bounds__(TM_NT) void tm_mem_fill_kernel(const u32 *__restrict__ ms_len, const u32 *__restrict__ ms_pos, u64 a,
                                                            u32 min_len, const u64 *__restrict__ offs, u64 slots,
                                                            u32 *__restrict__ mem_start, u32 *__restrict__ mem_pos,
                                                            u32 *__restrict__ mem_len) {
    __shared__ u32 s_scan[TM_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * TM_TILE + (u64)threadIdx.x * TM_ITEMS;
    u32 v[TM_ITEMS + 1];
    v[0] = base && base - 1 < a ? ms_len[base - 1] : 0u;
    u32 c = 0;
    for (u32 k = 0; k < TM_ITEMS; k++) {
        v[k + 1] = base + k < a ? ms_len[base + k] : 0u;
        c += base + k < a && tm_mem_is(v[k], v[k + 1], base + k, min_len) ? 1u : 0u;
    }
    u32 total;
    const u32 before = block_excl_sum<TM_NT>(c, s_scan, &total);
    u64 o = offs[blockIdx.x] + before;
    for (u32 k = 0; k < TM_ITEMS; k++) {
        if (base + k >= a || !tm_mem_is(v[k], v[k + 1], base + k, min_len) || o >= slots) continue;
        mem_start[o] = (u32)(base + k);
        mem_pos[o] = ms_pos[base + k];
        mem_len[o] = v[k + 1];
        o++;
    }
}
#endif  // TC_FM_MS_HOST_CHECK
