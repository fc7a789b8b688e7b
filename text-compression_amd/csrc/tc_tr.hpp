// tc_tr.hpp -- the runs (maximal repetitions, tandem repeats) of a text from two enhanced suffix arrays, the text's and
// its reverse's (included by tc_tr_host.hpp behind tc_lz_host.hpp, whose range minimum it instantiates for itself, and
// tc_fm_host.hpp, whose min tree and upward row search -- tc_fm_ms.hpp -- it uses unchanged).  No
// counterpart in the reference.  host/check/tr_kernels.cpp compiles tr_cand_kernel as plain C++ (TC_FM_MS_HOST_CHECK, as
// tc_fm_ms.hpp describes); the scatter, count, fill and order kernels are streaming passes and exist on the device only.
//
// include/textcomp.h defines a run (s, e, p).  N = n + 1; isa[i] = the suffix-array row of position i (isa[n] = 0, the
// empty suffix), lcp as tc_lcp_array defines it; isa_r / lcp_r the same of the reversed text.  Every run has a LYNDON
// ROOT: a length-p substring inside it that is a Lyndon word under the byte order or under its reverse, and the first
// position i of the leftmost such root is where the run is found.  In suffix terms, for position i < n and each of two
// orders
//   order 0   j = the smallest position > i with isa[j] < isa[i]   (always found: isa[n] = 0)
//   order 1   j = the smallest position > i with isa[j] > isa[i]   (none: no candidate)
// text[i .. j) is the longest Lyndon word that starts at i under that order, and p = j - i the only period a run rooted at i
// can have.  One isa serves both orders: order 1 is the reversed byte order, whose suffix order is the reverse of order
// 0's except where one suffix is a proper prefix of the other; the search for isa[j] > isa[i] takes such a j (isa[j] <
// isa[i]) for larger under order 1, that is, it puts the end of the text above every byte under order 1 where order 0 has
// it below -- the convention under which a run that touches the end of the text is found by exactly one of the two orders
// (held to the definition by brute force: host/check/tr_kernels.cpp).  "The smallest position behind i with a smaller value" is the
// upward search of tc_fm_ms.hpp over a min tree; level 0 of that tree is just a u32 array, so the tree built over isa
// answers order 0 and the one over N - 1 - isa[j] order 1.  Then, with i + p < n and text[i] = text[i + p],
//   e = the longest common prefix of the suffixes i and i + p: the minimum of lcp between their two rows
//   b = the longest common suffix of text[0 .. i) and text[0 .. i + p), 0 at i = 0: the same in the reversed text, between
//       the rows isa_r[n - i] and isa_r[n - i - p]
// and the candidate is a run iff b < p and b + e >= p: the run (i - b, i + p + e - 1, p).  b + e >= p: the stretch of period
// p around i is at least 2 p long.  b < p: no root of this run starts further left, so every run is found exactly once and
// nothing has to be deduplicated (without it the last positions of the text yield periods that are not the smallest).
// No lane walks the text: two searches, at most 2 TR_DIRECT bytes compared directly per candidate (where e or b is below
// TR_DIRECT that is the answer, and the range minimum between two rows that share so little -- rows far apart, a climb over
// every level -- is never asked) and at most four range minima of at most 2 f words per level each, whatever the text's
// periodicity.
//
// The output order is (start, period), which is not the order of i.  tr_cand_kernel writes one candidate word pair per
// (position, order); tr_count_kernel adds the kept ones up per start (a vector atomic); the scan of those counts gives
// every start its segment; tr_fill_kernel deals the segment's slots out in arrival order, and tr_order_kernel -- one lane
// per start with two or more runs -- sorts the segment by period.  The periods of runs that share a start are distinct
// (a start and a period determine the run) and grow at least like Fibonacci numbers, so a segment holds fewer than
// TR_SEG_MAX runs on any text the library takes; the result does not depend on the arrival order.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
// [0, 1: the search of order 0, 1; 2, 3: the range minimum of the text, of its reverse][the highest level it scanned]
static u64 tr_climbed[4][FM_MS_MAXLEV + 1] = {};
static u64 tr_seen_search[FM_MS_MAXLEV + 1] = {}, tr_seen_min[FM_MS_MAXLEV + 1] = {};
static inline void tr_note(u32 kind, const u64 *now, u64 *seen) {
    for (u32 lev = 0; lev <= FM_MS_MAXLEV; lev++) {
        tr_climbed[kind][lev] += now[lev] - seen[lev];
        seen[lev] = now[lev];
    }
}
#define TR_SEARCHED(o) tr_note(o, fm_ms_climbed[1], tr_seen_search)
#define TR_MINIMUM(k) tr_note(2u + (k), lz_climbed, tr_seen_min)
#else
#define TR_SEARCHED(o) ((void)0)
#define TR_MINIMUM(k) ((void)0)
#endif

#define TR_NT 256
#define TR_SEG_MAX 64u          // more runs than this share no start below 2^31 bytes (three-squares lemma)
#define TR_DIRECT 8u            // bytes compared directly each way before a range minimum is asked: a bound, not a walk

// what tc_tandem_repeats filters by
struct TrFilter {
    u32 min_period, max_period, min_copies, min_len;
};

// the minimum of lcp between the rows x and y of one ESA, x != y: the longest common prefix of their suffixes (two
// positions share no row, and no row is N or above: on any other content the answer is 0 and nothing is read)
FM_MS_DEVICE u32 tr_lce(const FmMsTree &L, u32 x, u32 y) {
    const u32 lo = x < y ? x : y, hi = x < y ? y : x;
    if (lo == hi || hi >= L.s_cnt[0]) return 0;
    return lz_range_min<2>(L, lo + 1u, hi);
}

// One lane per text position i < n.  Five arrays of N = n + 1 entries -- isa, comp = N - 1 - isa, lcp, isa_r, lcp_r -- and
// their min trees (fm_lmin_kernel, fan-out 2^lf), all of one shape.  Candidate (i, order) goes to slot 2 i + order:
// c_pl = period << 32 | length (0: none), c_start = the run's start.
FM_MS_KERNEL tr_cand_kernel(const u8 *__restrict__ text, u32 n, const u32 *__restrict__ isa, const u32 *__restrict__ isa_min,
                            const u32 *__restrict__ comp, const u32 *__restrict__ comp_min, const u32 *__restrict__ lcp,
                            const u32 *__restrict__ lcp_min, const u32 *__restrict__ isa_r, const u32 *__restrict__ lcp_r,
                            const u32 *__restrict__ lcp_r_min, u32 lf, TrFilter f, u32 *__restrict__ c_start,
                            u64 *__restrict__ c_pl) {
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    const u32 N = n + 1u;
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 i64 = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (i64 >= n) return;
    const u32 i = (u32)i64, ri = isa[i], ci = text[i];
    FmMsTree T;
    T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    for (u32 o = 0; o < 2; o++) {
        T.lcp = o ? comp : isa; T.lmin = o ? comp_min : isa_min;
        const u32 d = o ? N - 1u - ri : ri;                     // (order 0: ri >= 1, only the empty suffix has row 0)
        u32 start = 0;
        u64 pl = 0;
        const u32 j = d ? fm_ms_next_below(T, N, i, d) : N;     // (nothing is below 0)
        TR_SEARCHED(o);
        const u32 p = j - i;
        if (j < n && p >= f.min_period && (f.max_period == 0 || p <= f.max_period) && text[j] == ci) {
            // the first TR_DIRECT bytes each way are compared as bytes: on most texts most comparisons end there, and two
            // rows of one ESA that share only a byte or two lie far apart -- the dearest range minimum there is
            // b first, and no further than p: b = p says a root of this run starts further left, and inside a long run of a
            // short period that is nearly every position
            u32 e = 1, b = 0;
            const u32 bmax = p < TR_DIRECT ? p : TR_DIRECT;
            while (b < bmax && b < i && text[i - 1u - b] == text[j - 1u - b]) b++;
            if (b == TR_DIRECT && p > TR_DIRECT) {
                T.lcp = lcp_r; T.lmin = lcp_r_min;
                b = tr_lce(T, isa_r[n - i], isa_r[n - j]);
                TR_MINIMUM(1);
            }
            if (b < p) {
                while (e < TR_DIRECT && j + e < n && text[i + e] == text[j + e]) e++;
                if (e == TR_DIRECT) {
                    T.lcp = lcp; T.lmin = lcp_min;
                    e = tr_lce(T, ri, isa[j]);
                    TR_MINIMUM(0);
                }
                const u32 len = b + p + e;                      // (<= n: the run lies inside the text)
                if (b + e >= p && len / p >= f.min_copies && len >= f.min_len) {
                    start = i - b;
                    pl = (u64)p << 32 | len;
                }
            }
        }
        c_start[2 * i64 + o] = start;
        c_pl[2 * i64 + o] = pl;
    }
}

#ifndef TC_FM_MS_HOST_CHECK
// out[k] = in[n - 1 - k]
__global__ __launch_bounds__(TR_NT) void tr_reverse_kernel(const u8 *__restrict__ in, u32 n, u8 *__restrict__ out) {
    const u64 k = (u64)blockIdx.x * TR_NT + threadIdx.x;
    if (k < n) out[k] = in[n - 1u - k];
}

// isa[sa[r]] = r over the N rows
__global__ __launch_bounds__(TR_NT) void tr_isa_kernel(const u32 *__restrict__ sa, u32 N, u32 *__restrict__ isa, u32 *__restrict__ err) {
    const u64 r = (u64)blockIdx.x * TR_NT + threadIdx.x;
    if (r >= N) return;
    const u32 i = sa[r];
    if (i >= N) {               // (not on a suffix array)
        if (err) atomicOr(err, LCP_ERR_SA);
        return;
    }
    isa[i] = (u32)r;
}

// comp[j] = N - 1 - isa[j]: a streaming pass behind the scatter (a second scattered store in tr_isa_kernel cost 13 ms at
// 2^28 rows, this pass under 1)
__global__ __launch_bounds__(TR_NT) void tr_comp_kernel(const u32 *__restrict__ isa, u32 N, u32 *__restrict__ comp) {
    const u64 j = (u64)blockIdx.x * TR_NT + threadIdx.x;
    if (j < N) comp[j] = N - 1u - isa[j];
}

// cnt[s] += the candidates kept with start s (cnt: n words of 8 bytes, zero before the launch)
__global__ __launch_bounds__(TR_NT) void tr_count_kernel(const u32 *__restrict__ c_start, const u64 *__restrict__ c_pl, u64 slots,
                                                         u32 n, u64 *__restrict__ cnt) {
    const u64 k = (u64)blockIdx.x * TR_NT + threadIdx.x;
    if (k >= slots || !c_pl[k]) return;
    const u32 s = c_start[k];
    if (s < n) atomicAdd(reinterpret_cast<unsigned long long *>(cnt + s), 1ull);
}

// every kept candidate to a slot of its start's segment [offs[s], offs[s] + cnt[s]): cnt[s] counts down to 0, so the slot
// inside the segment is the arrival order; tr_order_kernel makes the order the text's own
__global__ __launch_bounds__(TR_NT) void tr_fill_kernel(const u32 *__restrict__ c_start, const u64 *__restrict__ c_pl, u64 slots,
                                                        u32 n, u64 *__restrict__ cnt, const u64 *__restrict__ offs, u64 total,
                                                        u32 *__restrict__ run_start, u32 *__restrict__ run_len,
                                                        u32 *__restrict__ run_period) {
    const u64 k = (u64)blockIdx.x * TR_NT + threadIdx.x;
    if (k >= slots) return;
    const u64 pl = c_pl[k];
    if (!pl) return;
    const u32 s = c_start[k];
    if (s >= n) return;
    const u64 left = atomicAdd(reinterpret_cast<unsigned long long *>(cnt + s), ~0ull);     // (minus one)
    const u64 o = offs[s] + left - 1u;
    if (left == 0 || o >= total) return;        // (more arrivals than were counted: not on one call's own words)
    run_start[o] = s;
    run_len[o] = (u32)pl;
    run_period[o] = (u32)(pl >> 32);
}

// one lane per start: a segment of two or more runs is put in increasing period (insertion sort; the start is the same)
__global__ __launch_bounds__(TR_NT) void tr_order_kernel(const u64 *__restrict__ offs, u32 n, u64 total, u32 *__restrict__ run_len,
                                                         u32 *__restrict__ run_period) {
    const u64 s = (u64)blockIdx.x * TR_NT + threadIdx.x;
    if (s >= n) return;
    const u64 lo = offs[s], hi = s + 1 < n ? offs[s + 1] : total;
    if (hi > total || hi < lo + 2) return;
    const u32 m = hi - lo < TR_SEG_MAX ? (u32)(hi - lo) : TR_SEG_MAX;
    for (u32 a = 1; a < m; a++) {
        const u32 p = run_period[lo + a], l = run_len[lo + a];
        u32 c = a;
        while (c > 0 && run_period[lo + c - 1] > p) {
            run_period[lo + c] = run_period[lo + c - 1];
            run_len[lo + c] = run_len[lo + c - 1];
            c--;
        }
        run_period[lo + c] = p;
        run_len[lo + c] = l;
    }
}
#endif  // TC_FM_MS_HOST_CHECK
