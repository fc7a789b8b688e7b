// tc_maw.hpp -- the minimal absent words of a text from its enhanced suffix array (included by tc_maw_host.hpp behind
// tc_rep_host.hpp, whose left-context change counts it uses, and tc_fm_host.hpp, whose min tree and row searches --
// tc_fm_ms.hpp -- it uses unchanged).  No counterpart in the reference.  host/check/maw_kernels.cpp
// compiles maw_row_body, maw_range_or and the two searches as plain C++ (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes);
// the tree build and the kernel around the body -- workgroup sums, the LDS histogram -- exist on the device only.
//
// include/textcomp.h defines a minimal absent word (MAW) x = a . w . b: x does not occur, a . w and w . b do.  N = n + 1
// rows, sa / lcp as tc_lcp_array defines them, left(r) = text[sa[r] - 1], Nothing for the row `primary` with sa = 0, and
// left(0) = text[n - 1] (that is what sa_build writes to L[0]).  A NODE is the root [0, N - 1] with l = 0 or an LCP interval
// [lb, rb] of depth l as tc_rep.hpp defines it; its BOUNDARIES are the rows k in (lb, rb] with lcp[k] = l, its CHILDREN the
// maximal row ranges between boundaries, the one that starts at lb dropped when sa[lb] + l = n (that suffix is w itself at
// the text's end: no next byte).  With Lw = the set of left(r) over the node and Lc the same over a child [cl, cr] whose
// next byte is b = text[sa[cl] + l], the words of the child are a . w . b for a in Lw \ Lc: a . w occurs (a is in Lw), w . b
// occurs (the child), a . w . b does not (a is not in Lc).  Their length is l + 2.
//
// One lane per row k >= 1, l = lcp[k]; k is a boundary of exactly one node:
//   l + 2 outside [min_len, max_len]: none, before any search
//   lb = the largest row <= k - 1 with lcp < l, rb = (the smallest row > k with lcp < l) - 1      (l = 0: the root, no search)
//   chg[rb] - chg[lb] = 0: all left contexts are equal, every Lc = Lw: none
//   q = the smallest row > k with lcp < l + 1: the lane owns the child [k, q - 1]
//   k is the node's first boundary iff the largest row <= k - 1 with lcp < l + 1 is lb (lb = k - 1: it is, no search): then
//   it also owns the first child [lb, k - 1], unless sa[lb] + l = n
//   Lw, and Lc of its one or two children, by range ORs; count = popcount(Lw & ~Lc) over them, at most 512
// The words of a row come out first child first, inside a child by increasing a; the list is in increasing k.
//
// A set is one u64 of dense byte codes when the text has at most 64 distinct bytes and four u64 indexed by the byte itself
// otherwise (WIDE), updated by selects as the set of rep_row_kernel<true> is.  The OR tree has the shape of the min tree
// (fm_ms_tree_shape): level 0 is the last column itself, entry j of level k + 1 is the OR of the entries [f j, f j + f) of
// level k.  A range OR takes the partial groups at both ends of its range, steps inside, and goes up: at most 2 f entries
// per level -- bytes at the bottom, sets above -- on any text.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_fm_ms.hpp"
// what host/check/maw_kernels.cpp asserts happened: [0] the first child was dropped (sa[lb] + l = n), [1] a child had an
// empty Lc (the primary row alone), [2] the chg exit fired, [3] the lb = k - 1 shortcut fired, [4] a lane had words for both
// of its children, [5] a wide set had members in all four words; maw_or_level[v]: range ORs whose highest level was v
static u64 maw_seen[6] = {};
static u64 maw_or_level[FM_MS_MAXLEV + 1] = {};
#define MAW_SEEN(k) (maw_seen[k]++)
#define MAW_OR_LEVEL(v) (maw_or_level[v]++)
#define MAW_UNROLL
#define MAW_UNROLL1
// bytes [i, i + 4) of the last column, i a multiple of 4, the byte of row i in the low bits; rows from N on read as 0
static inline u32 maw_load_bytes4(const u8 *L, u32 i, u32 N) {
    u32 w = 0;
    for (u32 k = 0; k < 4; k++) w |= i + k < N ? (u32)L[i + k] << (8 * k) : 0u;
    return w;
}
#else
#define MAW_SEEN(k) ((void)0)
#define MAW_OR_LEVEL(v) ((void)0)
#define MAW_UNROLL _Pragma("unroll")
#define MAW_UNROLL1 _Pragma("unroll 1")
// (the last column is carved with 16 spare bytes behind its N rows and starts 4-byte aligned)
FM_MS_DEVICE u32 maw_load_bytes4(const u8 *__restrict__ L, u32 i, u32) { return *reinterpret_cast<const u32 *>(L + i); }
#endif

#define MAW_MAX_KMAX 4096u      // the limit of tc_kmer_profile
enum { MAW_COUNT = 0, MAW_FILL = 1, MAW_HIST = 2 };

template <bool WIDE>
struct MawSet {
    u64 w[WIDE ? 4 : 1];
};
#define MAW_WORDS (WIDE ? 4u : 1u)

// what the lanes know of the text's enhanced suffix array and its two trees
struct MawArgs {
    const u32 *lcp, *lmin, *sa;
    const u64 *chg;             // the left-context change counts of rep_left_kernel + tc_scan64
    const u8 *L;                // the last column, N rows
    const u64 *ortree;          // level k >= 1 of the OR tree starts at word s_off[k] * (WIDE ? 4 : 1)
    u32 N, lf, primary, min_len, max_len;
    u64 alpha[4];               // bit v: the byte v occurs in the text
};
struct MawTree {
    const u8 *L;
    const u64 *ortree;
    const u32 *s_off;
    const u8 *s_code;           // byte -> dense code (not WIDE)
    u32 N, lf, primary;
};

// the dense code of the byte v: the number of smaller bytes that occur
FM_MS_HD u32 maw_code_of(const u64 *alpha, u32 v) {
    u32 c = 0;
    for (u32 i = 0; i < 4; i++) {
        const u64 m = i < (v >> 6) ? ~0ull : i == (v >> 6) ? (1ull << (v & 63u)) - 1ull : 0ull;
        c += (u32)__builtin_popcountll(alpha[i] & m);
    }
    return c;
}

template <bool WIDE>
FM_MS_DEVICE void maw_set_add(MawSet<WIDE> &s, u32 c) {
    const u64 bit = 1ull << (c & 63u);
    if (WIDE) {
        const u32 w = c >> 6;
MAW_UNROLL
        for (u32 i = 0; i < MAW_WORDS; i++) s.w[i] |= w == i ? bit : 0ull;
    } else {
        s.w[0] |= bit;
    }
}

// the rows x .. y of the last column, y - x < f: the primary row contributes nothing
template <bool WIDE>
FM_MS_DEVICE void maw_leaf_or(const MawTree &O, u32 x, u32 y, MawSet<WIDE> &s) {
    for (u32 c = x & ~3u; c <= y; c += 4) {
        const u32 w = maw_load_bytes4(O.L, c, O.N);
MAW_UNROLL
        for (u32 k = 0; k < 4; k++) {
            const u32 r = c + k, v = (w >> (8 * k)) & 255u;
            if (r < x || r > y || r == O.primary) continue;
            maw_set_add<WIDE>(s, WIDE ? v : (u32)O.s_code[v]);
        }
    }
}

// the OR of left(r) over the rows lo .. hi (lo <= hi < N)
template <bool WIDE>
FM_MS_DEVICE MawSet<WIDE> maw_range_or(const MawTree &O, u32 lo, u32 hi) {
    MawSet<WIDE> s;
MAW_UNROLL
    for (u32 i = 0; i < MAW_WORDS; i++) s.w[i] = 0;
    const u32 fmask = (1u << O.lf) - 1u;
    u32 lev = 0;
    while (true) {
        // entries lo .. hi of level lev: the rest of lo's group, the start of hi's group, the groups between one level up
        const u32 glo = lo >> O.lf, ghi = hi >> O.lf;
        const u32 e1 = glo == ghi ? hi : lo | fmask;
        if (lev == 0) {
            maw_leaf_or<WIDE>(O, lo, e1, s);
            if (glo != ghi) maw_leaf_or<WIDE>(O, hi & ~fmask, hi, s);
        } else {
            const u64 *lv = O.ortree + (u64)O.s_off[lev] * MAW_WORDS;
            for (u32 e = lo; e <= e1; e++) {
MAW_UNROLL
                for (u32 i = 0; i < MAW_WORDS; i++) s.w[i] |= lv[(u64)e * MAW_WORDS + i];
            }
            if (glo != ghi) {
                for (u32 e = hi & ~fmask; e <= hi; e++) {
MAW_UNROLL
                    for (u32 i = 0; i < MAW_WORDS; i++) s.w[i] |= lv[(u64)e * MAW_WORDS + i];
                }
            }
        }
        if (ghi <= glo + 1u) break;
        lo = glo + 1u;
        hi = ghi - 1u;
        lev++;
    }
    MAW_OR_LEVEL(lev);
    return s;
}

// The lane of row k, 1 <= k < N.  emit(first slot of the child inside the row's segment, cl, the set Lw \ Lc) once per child
// that has words, the first child first.  Returns the row's word count.
template <bool WIDE, class Emit>
FM_MS_DEVICE u32 maw_row_body(const MawArgs &P, const FmMsTree &T, const MawTree &O, u32 k, Emit &&emit) {
    const u32 N = P.N, n = N - 1u, l = P.lcp[k];
    if (l + 2u < P.min_len || (P.max_len != 0 && l + 2u > P.max_len)) return 0;     // (l < n <= TC_MAX_N: no overflow)
    u32 lb = 0, rb = N - 1u;
    if (l != 0) {                                   // (the searches need d >= 1; the root needs none)
        lb = fm_ms_prev_below(T, k - 1u, l);
        rb = fm_ms_next_below(T, N, k, l) - 1u;
    }
    if (rb <= lb || rb >= N) return 0;              // (not on an LCP array of a text: keeps every range inside the rows)
    if (P.chg[rb] - P.chg[lb] == 0) {
        MAW_SEEN(2);
        return 0;
    }
    u32 q = fm_ms_next_below(T, N, k, l + 1u);
    if (q <= k || q > rb + 1u) q = rb + 1u;         // (not on an LCP array of a text)
    bool first = lb == k - 1u;
    if (first) MAW_SEEN(3);
    else first = fm_ms_prev_below(T, k - 1u, l + 1u) == lb;
    if (first && (u64)P.sa[lb] + l >= n) {
        first = false;
        MAW_SEEN(0);
    }
    const MawSet<WIDE> Lw = maw_range_or<WIDE>(O, lb, rb);
#ifdef TC_FM_MS_HOST_CHECK
    u32 filled = 0;
    for (u32 i = 0; i < MAW_WORDS; i++) filled += Lw.w[i] ? 1u : 0u;
    if (filled == 4) MAW_SEEN(5);
#endif
    u32 total = 0;
MAW_UNROLL1
    for (u32 child = first ? 0u : 1u; child < 2u; child++) {
        const u32 cl = child ? k : lb, cr = child ? q - 1u : k - 1u;
        MawSet<WIDE> d = maw_range_or<WIDE>(O, cl, cr);
        u32 c = 0, any = 0;
MAW_UNROLL
        for (u32 i = 0; i < MAW_WORDS; i++) {
            any |= d.w[i] ? 1u : 0u;
            d.w[i] = Lw.w[i] & ~d.w[i];
            c += (u32)__builtin_popcountll(d.w[i]);
        }
        if (!any) MAW_SEEN(1);
        if (c) {
            if (total) MAW_SEEN(4);
            emit(total, cl, d);
        }
        total += c;
    }
    return total;
}

#ifndef TC_FM_MS_HOST_CHECK
// One level of the OR tree.  src = null: level 1 from the last column (dst[j] = the left bytes of the rows [f j, f j + f),
// without the primary row's); else dst[j] = the OR of src[f j .. min(f j + f, src_cnt)).
template <bool WIDE>
FM_MS_SMALL_KERNEL maw_tree_kernel(MawArgs P, const u64 *__restrict__ src, u32 src_cnt, u64 *__restrict__ dst, u32 dst_cnt) {
    __shared__ u8 s_code[256];
    if (!WIDE) s_code[threadIdx.x] = (u8)maw_code_of(P.alpha, threadIdx.x);
    __syncthreads();
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= dst_cnt) return;
    MawSet<WIDE> s;
MAW_UNROLL
    for (u32 i = 0; i < MAW_WORDS; i++) s.w[i] = 0;
    const u64 lo = (u64)j << P.lf, end = lo + (1u << P.lf);
    const u32 hi = (u32)((end < src_cnt ? end : src_cnt) - 1u);     // (lo < src_cnt: j < dst_cnt = ceil(src_cnt / f))
    if (!src) {
        MawTree O;
        O.L = P.L; O.ortree = nullptr; O.s_off = nullptr; O.s_code = s_code; O.N = P.N; O.lf = P.lf; O.primary = P.primary;
        maw_leaf_or<WIDE>(O, (u32)lo, hi, s);
    } else {
        for (u32 e = (u32)lo; e <= hi; e++) {
MAW_UNROLL
            for (u32 i = 0; i < MAW_WORDS; i++) s.w[i] |= src[(u64)e * MAW_WORDS + i];
        }
    }
MAW_UNROLL
    for (u32 i = 0; i < MAW_WORDS; i++) dst[(u64)j * MAW_WORDS + i] = s.w[i];
}

// One lane per row, a tile of FM_MS_NT rows per workgroup.
//   MAW_COUNT  rowcnt[k] = the words of row k, tilecnt[t] = those of the tile
//   MAW_FILL   the rows with rowcnt[k] > 0 run the body again and write their segments, from slot offs[t] + (the counts of
//              the tile's earlier rows) on; nothing at or behind slot `total` is written
//   MAW_HIST   hist[len] += the words of length len <= kmax, hist[kmax + 1] += the words of every length: an LDS histogram
//              of u32 counters (a tile has at most 256 * 512 words), one 64-bit atomic per non-zero bin and workgroup
template <bool WIDE, int MODE>
FM_MS_KERNEL maw_row_kernel(MawArgs P, u32 *__restrict__ rowcnt, u64 *__restrict__ tilecnt, const u64 *__restrict__ offs, u64 total,
                            u8 *__restrict__ maw_left, u32 *__restrict__ maw_pos, u32 *__restrict__ maw_len,
                            u64 *__restrict__ hist, u32 kmax) {
    __shared__ u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    __shared__ u32 s_scan[FM_MS_NT / 64 + 1];
    __shared__ u8 s_code[WIDE ? 1 : 256], s_byte[WIDE ? 1 : 64];
    __shared__ u32 s_hist[MODE == MAW_HIST ? MAW_MAX_KMAX + 1 : 1];
    if (threadIdx.x == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(P.N, P.lf, s_off, s_cnt, &words);
    }
    if (!WIDE) {
        const u32 v = threadIdx.x, c = maw_code_of(P.alpha, v);
        s_code[v] = (u8)c;
        if (P.alpha[v >> 6] >> (v & 63u) & 1ull) s_byte[c & 63u] = (u8)v;
    }
    if (MODE == MAW_HIST) {
        for (u32 i = threadIdx.x; i <= kmax; i += FM_MS_NT) s_hist[i] = 0;
    }
    __syncthreads();
    const u64 k64 = (u64)blockIdx.x * FM_MS_NT + threadIdx.x;
    const bool live = k64 >= 1 && k64 < P.N;
    const u32 k = (u32)k64;
    FmMsTree T;
    T.lcp = P.lcp; T.lmin = P.lmin; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = P.lf;
    MawTree O;
    O.L = P.L; O.ortree = P.ortree; O.s_off = s_off; O.s_code = s_code; O.N = P.N; O.lf = P.lf; O.primary = P.primary;
    u32 c = 0, tile_total;
    if (MODE == MAW_FILL) {
        c = live ? rowcnt[k] : 0u;
        const u64 o = offs[blockIdx.x] + block_excl_sum<FM_MS_NT>(c, s_scan, &tile_total);
        if (!c) return;
        const u32 len = P.lcp[k] + 2u;
        maw_row_body<WIDE>(P, T, O, k, [&](u32 at, u32 cl, MawSet<WIDE> d) {
            const u32 pos = P.sa[cl];
            u64 slot = o + at;
MAW_UNROLL
            for (u32 i = 0; i < MAW_WORDS; i++) {
                u64 m = d.w[i];
                while (m) {
                    const u32 b = (u32)__builtin_ctzll(m);
                    m &= m - 1ull;
                    if (slot >= total) return;
                    maw_left[slot] = WIDE ? (u8)(64u * i + b) : s_byte[b];
                    maw_pos[slot] = pos;
                    maw_len[slot] = len;
                    slot++;
                }
            }
        });
        return;
    }
    if (live) c = maw_row_body<WIDE>(P, T, O, k, [](u32, u32, MawSet<WIDE>) {});
    if (MODE == MAW_COUNT) {
        if (k64 < P.N) rowcnt[k] = c;
    } else if (c) {
        const u32 len = P.lcp[k] + 2u;
        if (len <= kmax) atomicAdd(&s_hist[len], c);
    }
    block_excl_sum<FM_MS_NT>(c, s_scan, &tile_total);
    if (MODE == MAW_COUNT) {
        if (threadIdx.x == 0) tilecnt[blockIdx.x] = tile_total;
        return;
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i <= kmax; i += FM_MS_NT) {
        const u32 v = s_hist[i];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(hist + i), (unsigned long long)v);
    }
    if (threadIdx.x == 0 && tile_total) atomicAdd(reinterpret_cast<unsigned long long *>(hist + kmax + 1u), (unsigned long long)tile_total);
}
#endif  // TC_FM_MS_HOST_CHECK
