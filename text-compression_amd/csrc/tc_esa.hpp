// tc_esa.hpp -- batched substring queries on a kept enhanced suffix array: longest common extension with mismatches, the
// suffix-array interval and the earliest occurrence of a substring of the text, and the order of two substrings (included by
// tc_esa_host.hpp behind tc_cov_host.hpp; it uses the min tree and the row searches of tc_fm_ms.hpp and the range minimum of
// tc_lz.hpp unchanged).  No counterpart in the reference.
// host/check/esa_kernels.cpp compiles the three kernels as plain C++ (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes).
//
// include/textcomp.h defines the three answers.  N = n + 1 rows; sa, lcp as tc_lcp_array defines them, isa[sa[r]] = r; T the min
// tree of lcp, S that of sa (one shape).  One lane per query, no lane walks over the text or over rows:
//   step    the longest common prefix of the suffixes a != b, clamped to lim >= 1 (a + lim <= n, b + lim <= n): the ESA_DIRECT
//           bytes of both come by two aligned 8-byte loads each, inside the handle's padded copy of the text (as 16 byte loads
//           the step ran at 3.6 G queries/s on random pairs; DESIGN.md has the figure of these), and are compared up to the
//           clamp -- never a byte at or behind it.  On most texts most extensions end there; two rows that share only a byte
//           or two lie far apart, the dearest range minimum there is (tc_tr.hpp).  Only where all ESA_DIRECT bytes agree and
//           the clamp lies further: two reads of isa and one lz_range_min over T between the two rows.
//   lce     bound = n - max(a, b); at most m + 1 steps (kangaroo jumps), each followed by the one mismatch it ran into.  Every
//           mismatch counts, a trailing one too: len is the largest L within the bound with at most m mismatches before L.
//   find    r = isa[start]; the rows of text[start .. start + len) are [lo, hi), lo = the nearest row at or above r with
//           lcp < len (fm_ms_prev_below), hi = the nearest row below r with lcp < len (fm_ms_next_below); the earliest
//           occurrence is the minimum of sa[lo .. hi): one lz_range_min over S.
//   compare one step clamped to min(a_len, b_len); short of the clamp one byte of each decides, at the clamp the lengths do.
// A query that leaves the text sets *bad and reads nothing; its outputs are not written.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
// what host/check/esa_kernels.cpp asserts happened: [0] a direct compare decided a step, [1] a range minimum decided one,
// [2] a range minimum was cut by the clamp, [3] a direct compare ended at the clamp, [4] a lane took all m + 1 steps,
// [5] a == b, [6] a bound of 0 (position n), [7] len = 0 in find, [8] a query refused
static u64 esa_seen[9] = {};
#define ESA_SEEN(k) (esa_seen[k]++)
#else
#define ESA_SEEN(k) ((void)0)
#endif

#define ESA_DIRECT 8u           // bytes compared directly before a range minimum is asked: a bound, not a walk
#define ESA_MAX_MISMATCH 16u    // TC_ESA_MAX_MISMATCH of include/textcomp.h

// the 8 bytes text[a .. a + 8), byte k in bits 8 k, by two aligned 8-byte loads: they end before (a & ~7) + 16 <= n + 16 for
// a < n, inside the padded copy the handle keeps (what lies behind the text is masked by the caller, never compared)
FM_MS_DEVICE u64 esa_load8(const u8 *__restrict__ text, u32 a) {
    const u32 sh = 8u * (a & 7u);
    u64 lo, hi;
#ifdef TC_FM_MS_HOST_CHECK
    memcpy(&lo, text + (a & ~7u), 8);
    memcpy(&hi, text + (a & ~7u) + 8, 8);
#else
    const u64 *w = reinterpret_cast<const u64 *>(text + (a & ~7u));     // (the handle's text starts a hipMalloc block)
    lo = w[0];
    hi = w[1];
#endif
    return sh ? lo >> sh | hi << (64u - sh) : lo;
}

// min(lim, the longest common prefix of the suffixes a and b), a != b, lim >= 1, a + lim <= n and b + lim <= n
FM_MS_DEVICE u32 esa_step(const u8 *__restrict__ text, const u32 *__restrict__ isa, const FmMsTree &T, u32 a, u32 b, u32 lim) {
    const u32 dmax = lim < ESA_DIRECT ? lim : ESA_DIRECT;
    const u64 keep = dmax < 8u ? (1ull << (8u * dmax)) - 1ull : ~0ull;     // the bytes before the clamp
    const u64 va = esa_load8(text, a) & keep, vb = esa_load8(text, b) & keep;
    const u64 x = va ^ vb;
    u32 e = x ? (u32)__builtin_ctzll(x) >> 3 : dmax;
    if (e == ESA_DIRECT && lim > ESA_DIRECT) {
        const u32 ra = isa[a], rb = isa[b];
        const u32 lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        // (two positions share no row, and no row is N or above: on any other content the direct bytes are the answer)
        if (lo < hi && hi < T.s_cnt[0]) e = lz_range_min<6>(T, lo + 1u, hi);
        ESA_SEEN(1);
        if (e > lim) {
            e = lim;
            ESA_SEEN(2);
        }
    } else {
        ESA_SEEN(0);
        if (e == lim) ESA_SEEN(3);
    }
    return e;
}

// the shape of the trees over N rows into LDS, and the tree of one level-0 array
#define ESA_TREE_SHAPE(N, lf)                                                            \
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;           \
    if (fm_ms_tid() == 0) {                                                              \
        u32 words;                                                                       \
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);                          \
    }                                                                                    \
    fm_ms_sync()

// One lane per query q < nq: len[q] = the largest L with a + L <= n, b + L <= n and at most m mismatching k < L; mm[q] (may be
// null) = those mismatches.  Positions 0 .. n; a == b answers n - a.  m <= ESA_MAX_MISMATCH.
FM_MS_KERNEL esa_lce_kernel(const u8 *__restrict__ text, u32 n, const u32 *__restrict__ isa, const u32 *__restrict__ lcp,
                            const u32 *__restrict__ lcp_min, u32 lf, const u32 *__restrict__ qa, const u32 *__restrict__ qb, u64 nq,
                            u32 m, u32 *__restrict__ len, u32 *__restrict__ mm, u32 *__restrict__ bad) {
    ESA_TREE_SHAPE(n + 1u, lf);
    const u64 q = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (q >= nq) return;
    const u32 a = qa[q], b = qb[q];
    if (a > n || b > n) {
        ESA_SEEN(8);
        bad[0] = 1u;
        return;
    }
    FmMsTree T;
    T.lcp = lcp; T.lmin = lcp_min; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    const u32 bound = n - (a > b ? a : b);
    u32 R = 0, turn = 0;
    if (a == b) {
        ESA_SEEN(5);
        R = bound;
    }
    if (bound == 0) ESA_SEEN(6);
    while (R < bound) {
        R += esa_step(text, isa, T, a + R, b + R, bound - R);
        if (turn == m) ESA_SEEN(4);
        if (R >= bound || turn == m) break;
        R++;                                        // position R is a mismatch
        turn++;
    }
    len[q] = R;
    if (mm) mm[q] = turn;
}

// One lane per query q < nq over the substring text[start .. start + len): first_row[q] = the first row whose suffix starts
// with it, occ[q] = the number of such rows, first_pos[q] = the smallest position where it occurs; each may be null.  len = 0
// answers (0, N, 0).
FM_MS_KERNEL esa_find_kernel(u32 n, const u32 *__restrict__ sa, const u32 *__restrict__ isa, const u32 *__restrict__ lcp,
                             const u32 *__restrict__ sa_min, const u32 *__restrict__ lcp_min, u32 lf, const u32 *__restrict__ qs,
                             const u32 *__restrict__ ql, u64 nq, u32 *__restrict__ first_row, u32 *__restrict__ occ,
                             u32 *__restrict__ first_pos, u32 *__restrict__ bad) {
    const u32 N = n + 1u;
    ESA_TREE_SHAPE(N, lf);
    const u64 q = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (q >= nq) return;
    const u32 s = qs[q], l = ql[q];
    if (s > n || l > n - s) {
        ESA_SEEN(8);
        bad[0] = 1u;
        return;
    }
    u32 lo = 0, hi = N, pos = 0;
    if (l) {
        FmMsTree T;
        T.lcp = lcp; T.lmin = lcp_min; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
        const u32 r = isa[s];                       // (s < n: l >= 1)
        if (r >= N) return;                         // (not on an inverse suffix array)
        lo = fm_ms_prev_below(T, r, l);
        hi = fm_ms_next_below(T, N, r, l);
        if (first_pos) {
            T.lcp = sa; T.lmin = sa_min;
            pos = hi > lo ? lz_range_min<6>(T, lo, hi - 1u) : s;
        }
    } else {
        ESA_SEEN(7);
    }
    if (first_row) first_row[q] = lo;
    if (occ) occ[q] = hi - lo;
    if (first_pos) first_pos[q] = pos;
}

// One lane per query q < nq: order[q] = -1, 0, 1 as text[a .. a + la) sorts before, equals, sorts behind text[b .. b + lb)
// (bytes as unsigned, a proper prefix first); common[q] (may be null) = the length of their common prefix.
FM_MS_KERNEL esa_compare_kernel(const u8 *__restrict__ text, u32 n, const u32 *__restrict__ isa, const u32 *__restrict__ lcp,
                                const u32 *__restrict__ lcp_min, u32 lf, const u32 *__restrict__ qa, const u32 *__restrict__ qla,
                                const u32 *__restrict__ qb, const u32 *__restrict__ qlb, u64 nq, signed char *__restrict__ order,
                                u32 *__restrict__ common, u32 *__restrict__ bad) {
    ESA_TREE_SHAPE(n + 1u, lf);
    const u64 q = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (q >= nq) return;
    const u32 a = qa[q], la = qla[q], b = qb[q], lb = qlb[q];
    if (a > n || la > n - a || b > n || lb > n - b) {
        ESA_SEEN(8);
        bad[0] = 1u;
        return;
    }
    FmMsTree T;
    T.lcp = lcp; T.lmin = lcp_min; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    const u32 lim = la < lb ? la : lb;
    u32 c = lim;
    if (a == b) ESA_SEEN(5);
    if (a != b && lim) c = esa_step(text, isa, T, a, b, lim);
    int o;
    if (c < lim) o = text[a + c] < text[b + c] ? -1 : 1;
    else o = la < lb ? -1 : (la > lb ? 1 : 0);
    order[q] = (signed char)o;
    if (common) common[q] = c;
}
