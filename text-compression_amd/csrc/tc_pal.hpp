// tc_pal.hpp -- the palindromes and inverted repeats of a text, with mismatches, from one enhanced suffix array of the text
// joined to its own mirror image (included by tc_pal_host.hpp behind tc_tr_host.hpp, whose inverse-array scatter it uses,
// tc_lz_host.hpp, whose range minimum it instantiates for itself, and tc_fm_host.hpp, whose min tree -- tc_fm_ms.hpp -- it
// uses unchanged).  No counterpart in the reference.  host/check/pal_kernels.cpp compiles
// pal_centre_kernel as plain C++ (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes); the joint-text, count, fill and
// longest kernels are streaming passes and exist on the device only.
//
// include/textcomp.h defines a palindrome under a byte involution sigma.  S = text . sigma(reverse(text)), 2n bytes, no
// separator (all 256 byte values stay legal): S[n + j] = sigma(text[n - 1 - j]), so text position l has its image at
// S[2n - 1 - l].  N = 2n + 1 rows; isa[i] = the suffix-array row of position i of S, lcp as tc_lcp_array defines it.  For a
// centre c in 0 .. 2n - 2 let l0 = c / 2, r0 = (c + 1) / 2: the pairs of the palindromes centred there are (l0 - k, r0 + k),
// k = 0 .. bound - 1 with bound = min(l0 + 1, n - r0), and pair k matches iff S[r0 + k] = S[2n - 1 - l0 + k].  So the pairs
// from R on match for as long as the suffixes r0 + R and 2n - 1 - l0 + R of S share a prefix -- one longest common extension,
// the minimum of lcp between their two rows.  What the missing separator costs: the common prefix may run on past the
// text's edge (on a unary text it nearly always does), so every extension is clamped to bound - R.
//
// One lane per centre, at most m + 1 turns (kangaroo jumps), no walk over the text:
//   e = min(LCE(r0 + R, 2n - 1 - l0 + R), bound - R);  e > 0: R += e, and (R, turn) is remembered: the outermost pair of
//   the first R matches and `turn` of them do not;  R = bound: done;  otherwise pair R is a mismatch: R += 1, next turn.
// The remembered (R, mm) is the longest palindrome at c with at most m mismatches whose outermost pair matches: a longer
// one would need a matching pair behind the m-th mismatch's successor run, which the last turn covered.  Trailing
// mismatches are dropped by remembering, not by scanning.  len = 2 R - 1 + (c & 1); start = l0 - R + 1.
// Each LCE first compares up to PAL_DIRECT bytes directly (never past the clamp): on most texts most extensions end
// there, and two rows that share only a byte or two lie far apart -- the dearest range minimum there is (tc_tr.hpp).
//
// word[c] = len << 32 | mm, 0 for none or for len < min_len: one 8-byte store per centre.  The list is the non-zero words
// in centre order: pal_count_kernel counts them per tile, the scan of the tiles' counts gives every tile its first slot,
// pal_fill_kernel scans inside the tile and writes -- no atomics, the order is the centres'.  The longest palindrome is one
// reduction over (len << 32 | ~c): the largest len, of its centres the smallest.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
// what host/check/pal_kernels.cpp asserts happened: [0] a range minimum was cut by the clamp, [1] a direct compare ended at
// the clamp, [2] a lane used all m + 1 turns, [3] a trailing mismatch was dropped, [4] a direct compare decided an
// extension, [5] a range minimum decided one
static u64 pal_seen[6] = {};
#define PAL_SEEN(k) (pal_seen[k]++)
#else
#define PAL_SEEN(k) ((void)0)
#endif

#define PAL_NT 256
#define PAL_ITEMS 8u            // centres per lane of the count and fill kernels
#define PAL_TILE (PAL_NT * PAL_ITEMS)
#define PAL_DIRECT 8u           // bytes compared directly before a range minimum is asked: a bound, not a walk
#define PAL_MAX_MISMATCH 16u    // TC_PAL_MAX_MISMATCH of include/textcomp.h

// the minimum of lcp between the rows x and y of the ESA, x != y: the longest common prefix of their suffixes (two
// positions share no row, and no row is N or above: on any other content the answer is 0 and nothing is read)
FM_MS_DEVICE u32 pal_lce(const FmMsTree &L, u32 x, u32 y) {
    const u32 lo = x < y ? x : y, hi = x < y ? y : x;
    if (lo == hi || hi >= L.s_cnt[0]) return 0;
    return lz_range_min<3>(L, lo + 1u, hi);
}

// One lane per centre c < 2n - 1 (n >= 1, 2n + 1 rows).  S: the joint text, 2n bytes; isa, lcp: N = 2n + 1 entries;
// lcp_min: the min tree over lcp (fm_lmin_kernel, fan-out 2^lf).  m <= PAL_MAX_MISMATCH, min_len >= 1.
FM_MS_KERNEL pal_centre_kernel(const u8 *__restrict__ S, u32 n, const u32 *__restrict__ isa, const u32 *__restrict__ lcp,
                               const u32 *__restrict__ lcp_min, u32 lf, u32 m, u32 min_len, u64 *__restrict__ word) {
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    const u32 N = 2u * n + 1u;
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 c64 = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (c64 + 1u >= 2ull * n) return;
    const u32 c = (u32)c64, l0 = c >> 1, r0 = (c + 1u) >> 1;
    const u32 bound = l0 + 1u < n - r0 ? l0 + 1u : n - r0;      // (>= 1: r0 <= n - 1)
    const u32 a0 = r0, b0 = 2u * n - 1u - l0;                   // (a0 + k <= n - 1 < n <= b0 + k <= 2n - 1 for k < bound)
    FmMsTree T;
    T.lcp = lcp; T.lmin = lcp_min; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    u32 R = 0, best = 0, mm = 0, turn = 0;
    while (true) {
        const u32 lim = bound - R, a = a0 + R, b = b0 + R;      // (lim >= 1)
        const u32 dmax = lim < PAL_DIRECT ? lim : PAL_DIRECT;
        u32 e = 0;
        while (e < dmax && S[a + e] == S[b + e]) e++;
        if (e == PAL_DIRECT && lim > PAL_DIRECT) {
            e = pal_lce(T, isa[a], isa[b]);
            PAL_SEEN(5);
            if (e > lim) {
                e = lim;
                PAL_SEEN(0);
            }
        } else {
            PAL_SEEN(4);
            if (e == lim) PAL_SEEN(1);
        }
        if (e) {
            R += e;
            best = R;
            mm = turn;
        }
        if (turn == m) PAL_SEEN(2);
        if (R >= bound || turn == m) break;
        R++;                                                    // pair R is a mismatch
        turn++;
        if (R >= bound) break;
    }
    if (best && R > best) PAL_SEEN(3);
    const u32 len = 2u * best - 1u + (c & 1u);
    word[c] = best && len >= min_len ? (u64)len << 32 | mm : 0;
}

#ifndef TC_FM_MS_HOST_CHECK
// S = text . sigma(reverse(text)): out[k] = text[k], out[n + k] = sigma(text[n - 1 - k]), the table in LDS
__global__ __launch_bounds__(PAL_NT) void pal_joint_kernel(const u8 *__restrict__ text, u32 n, const u8 *__restrict__ sigma,
                                                           u8 *__restrict__ out) {
    __shared__ u8 s_sigma[256];
    s_sigma[threadIdx.x] = sigma[threadIdx.x];
    __syncthreads();
    const u64 k = (u64)blockIdx.x * PAL_NT + threadIdx.x;
    if (k >= n) return;
    out[k] = text[k];
    out[n + k] = s_sigma[text[n - 1u - k]];
}

// cnt[t] = the non-zero words of tile t (PAL_TILE centres, PAL_ITEMS consecutive ones per lane)
__global__ __launch_bounds__(PAL_NT) void pal_count_kernel(const u64 *__restrict__ word, u64 centres, u64 *__restrict__ cnt) {
    __shared__ u32 smem[PAL_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * PAL_TILE + (u64)threadIdx.x * PAL_ITEMS;
    u32 mine = 0, total;
    for (u32 k = 0; k < PAL_ITEMS; k++)
        if (base + k < centres && word[base + k]) mine++;
    block_excl_sum<PAL_NT>(mine, smem, &total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// the non-zero words of tile t to the slots from offs[t] on, in centre order (pal_mm may be null)
__global__ __launch_bounds__(PAL_NT) void pal_fill_kernel(const u64 *__restrict__ word, u64 centres, const u64 *__restrict__ offs,
                                                          u64 total, u32 *__restrict__ pal_start, u32 *__restrict__ pal_len,
                                                          u32 *__restrict__ pal_mm) {
    __shared__ u32 smem[PAL_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * PAL_TILE + (u64)threadIdx.x * PAL_ITEMS;
    u64 w[PAL_ITEMS];
    u32 mine = 0, tile_total;
#pragma unroll
    for (u32 k = 0; k < PAL_ITEMS; k++) {
        w[k] = base + k < centres ? word[base + k] : 0;
        if (w[k]) mine++;
    }
    u64 o = offs[blockIdx.x] + block_excl_sum<PAL_NT>(mine, smem, &tile_total);
#pragma unroll
    for (u32 k = 0; k < PAL_ITEMS; k++) {
        if (!w[k]) continue;
        if (o >= total) return;                 // (more words than were counted: not on one call's own words)
        const u32 len = (u32)(w[k] >> 32);
        pal_start[o] = (u32)((base + k + 1u - len) >> 1);       // c = 2 s + len - 1
        pal_len[o] = len;
        if (pal_mm) pal_mm[o] = (u32)w[k];
        o++;
    }
}

// out2[0] = max over centres of (len << 32 | ~c): the longest palindrome, and of its centres the smallest; out2[1] = the
// number of palindromes.  Both zeroed before the launch.  Any grid of LCP_NT lanes: the lanes stride over the centres.
// (the reduction of lcp_summary_kernel, over packed words)
__global__ __launch_bounds__(LCP_NT) void pal_longest_kernel(const u64 *__restrict__ word, u64 centres, u64 *__restrict__ out2) {
    __shared__ u64 smem[2 * (LCP_NT / 64) + 2];
    u64 key = 0, sum = 0;
    const u64 stride = (u64)gridDim.x * LCP_NT;
    for (u64 c = (u64)blockIdx.x * LCP_NT + threadIdx.x; c < centres; c += stride) {
        const u64 w = word[c];
        if (!w) continue;
        const u64 k = (w & 0xffffffff00000000ull) | (u64)(0xffffffffu - (u32)c);
        key = k > key ? k : key;
        sum++;
    }
    lcp_summary_publish(key, sum, smem, out2);
}
#endif  // TC_FM_MS_HOST_CHECK
