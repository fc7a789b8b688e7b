// tc_lz.hpp -- the LPF array and the LZ77 parse of a text against itself, and the inverse of the parse (included by
// tc_lz_host.hpp behind tc_fm_host.hpp, whose min tree and row searches -- tc_fm_ms.hpp -- it uses unchanged; DESIGN.md
// section 4.6).  No counterpart in the reference.  host/check/lz_kernels.cpp compiles lz_lpf_kernel and lz_range_min as
// plain C++ (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes); the tile kernels and the unparse rounds need barriers
// between lanes and exist on the device only.
//
// lpf[i] = the longest common prefix of suffix i with any suffix that starts before i; src[i] = where that suffix starts.
// Among the suffixes that start before i, suffix i has two lexicographic neighbours, and one of them attains the maximum:
// in suffix-array terms, with r the row of i, they are p = the nearest row above r and q = the nearest row below r whose
// sa is smaller than i, and the prefixes shared with them are min lcp[p + 1 .. r] and min lcp[r + 1 .. q].  "The nearest
// row with a smaller value" is the search tc_fm_ms.hpp runs over its min tree of the LCP array: level 0 of that tree is
// just a u32 array, so the same tree built over sa answers it (sa[0] = n is below no i, so row 0 never qualifies: a
// downward search that comes back with 0 found nothing).  The two range minima go over the tree of the LCP array:
// lz_range_min below.  On a tie the smaller neighbour (p) is taken; where lpf is 0, src is 0.
//
// The parse: next[i] = i + max(1, lpf[i]); the phrases start at the positions on the path from 0.  No lane walks that
// path over the text:
//   a  per tile of `tile` positions, next is pointer-jumped in LDS (two u32 buffers; a value at or behind the tile's end
//      no longer jumps) to exit[i] = the first position at or behind the tile's end that is reachable from i;
//   b  one lane follows exit from 0 and writes every tile's entry position (LZ_NONE for a tile a long phrase skips): at
//      most n / tile dependent reads;
//   c  per tile, from its entry, the path inside the tile is marked by doubling in LDS: every marked position marks
//      jump[i], then jump = jump o jump; after log2(tile) rounds every position of the path is marked; the marks are
//      counted;
//   d  behind the scan of the tiles' counts the same marking runs again and writes the phrases in position order: no
//      atomics, a deterministic order.
// The inverse: an exclusive scan of max(len, 1) gives the phrases' starts; a list is refused before anything is written
// (a copy whose source is not strictly before its own start, a literal above 255); then parent[i] = src + (i - start)
// for a copied byte and i itself for a literal, parent = parent o parent until nothing changes (parent[i] < i for every
// copied byte, so at most ceil(log2 n) + 1 rounds), and out[i] = out[parent[i]].
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_fm_ms.hpp"
static u64 lz_climbed[FM_MS_MAXLEV + 1] = {};   // [the highest level a range minimum scanned]
#define LZ_CLIMBED(lev) (lz_climbed[lev]++)
#else
#define LZ_CLIMBED(lev) ((void)0)
#endif

#define LZ_TILE 8192            // positions per tile of the parse: 9 bytes of LDS each, two workgroups per CU
#define LZ_TILE_MAX 16384       // the largest tile tc_dbg_lz_set_tile takes (144 KB of LDS)
#define LZ_NT 1024
#define LZ_NONE 0xffffffffu

// the minimum of m and of the entries [lo, hi] of one level (cnt entries; lo <= hi < cnt), by 16-byte loads
FM_MS_DEVICE u32 lz_scan_min(const u32 *lv, u32 cnt, u32 lo, u32 hi, u32 m) {
    for (u32 c = lo & ~3u; c <= hi; c += 4) {
        const FmMsQuad q = fm_ms_load4(lv, c, cnt);
        for (u32 k = 0; k < 4; k++) m = (c + k >= lo && c + k <= hi && q.v[k] < m) ? q.v[k] : m;
    }
    return m;
}

// the minimum of rows [lo, hi] of the tree's level 0, lo <= hi < N.  While the range spans groups, the rest of lo's
// group and the start of hi's are scanned and the range moves up to the groups strictly between: at most 2 f words per
// level and ceil(log_f N) levels on any text.  (No level above T.nlev is used: the top level is one group.)
// USER: an instance per calling file (0: lz_lpf_kernel, 1: tm_row_kernel of tc_tm.hpp, 2: tr_cand_kernel of tc_tr.hpp,
// 3: pal_centre_kernel of tc_pal.hpp, 4: sus_point_kernel of tc_sus.hpp, 5: cov_seed_kernel of tc_cov.hpp, 6: the three query
// kernels of tc_esa.hpp, 7: esx_match_kernel of tc_esa_xdoc.hpp).  The function is not inlined, so
// what the compiler knows of its callers shapes it: shared with tm_row_kernel, the one instance cost lz_lpf_kernel two more
// VGPRs (36 -> 38 in the resource listing); with an instance of its own, lz_lpf_kernel is compiled as it was.
template <int USER = 0>
FM_MS_SEARCH lz_range_min(const FmMsTree T, u32 lo, u32 hi) {
    const u32 fmask = (1u << T.lf) - 1u;
    u32 m = 0xffffffffu, lev = 0;
    while (true) {
        const u32 *lv = fm_ms_level(T, lev);
        const u32 cnt = T.s_cnt[lev];
        if ((lo >> T.lf) == (hi >> T.lf) || lev == T.nlev) {
            m = lz_scan_min(lv, cnt, lo, hi, m);
            break;
        }
        m = lz_scan_min(lv, cnt, lo, lo | fmask, m);
        m = lz_scan_min(lv, cnt, hi & ~fmask, hi, m);
        lo = (lo >> T.lf) + 1u;
        hi = (hi >> T.lf) - 1u;
        if (lo > hi || m == 0) break;
        lev++;
    }
    LZ_CLIMBED(lev);
    return m;
}

// One lane per suffix-array row r >= 1.  sa_min / lcp_min: the min trees (fm_lmin_kernel, fan-out 2^lf) over sa and
// lcp, both of N = n + 1 entries and so of one shape.  pack[i] = src << 32 | lpf: one 8-byte store per row.
FM_MS_KERNEL lz_lpf_kernel(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, const u32 *__restrict__ sa_min,
                           const u32 *__restrict__ lcp_min, u32 N, u32 lf, u64 *__restrict__ pack) {
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 r64 = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid() + 1u;
    if (r64 >= N) return;
    const u32 r = (u32)r64, i = sa[r];
    if (i >= N - 1u) return;                    // (not on a suffix array: rows 1 .. n hold the positions 0 .. n - 1)
    u32 lpf = 0, src = 0;
    if (i) {                                    // (the searches need d >= 1; nothing starts before position 0)
        FmMsTree S, L;
        S.lcp = sa; S.lmin = sa_min; S.s_off = s_off; S.s_cnt = s_cnt; S.nlev = s_nlev; S.lf = lf;
        L = S;
        L.lcp = lcp; L.lmin = lcp_min;
        const u32 p = fm_ms_prev_below(S, r - 1u, i);       // 0: no smaller neighbour
        const u32 q = fm_ms_next_below(S, N, r, i);         // N: no larger neighbour
        const u32 lp = p ? lz_range_min(L, p + 1u, r) : 0u;
        const u32 lq = q < N ? lz_range_min(L, r + 1u, q) : 0u;
        if (lp >= lq) {
            lpf = lp;
            src = lp ? sa[p] : 0u;
        } else {
            lpf = lq;
            src = sa[q];
        }
    }
    pack[i] = (u64)src << 32 | lpf;
}

#ifndef TC_FM_MS_HOST_CHECK
// pack -> the two arrays of tc_lpf_array (src may be null)
__global__ __launch_bounds__(256) void lz_unpack_kernel(const u64 *__restrict__ pack, u32 n, u32 *__restrict__ lpf,
                                                        u32 *__restrict__ src) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 v = pack[i];
    lpf[i] = (u32)v;
    if (src) src[i] = (u32)(v >> 32);
}

// Steps a, c and d of the parse, one workgroup per tile of `tile` = 2^ltile positions (64 .. LZ_TILE_MAX).  Dynamic LDS:
// two jump buffers of `tile` words and `tile` mark bytes.  A jump value is relative to the tile's first position; one
// at or above tlen (the tile's positions inside the text) has left the tile and stays as it is.
//   MODE 0  exitp[i] = the absolute position where the path from i leaves the tile (<= n)
//   MODE 1  cnt[t] = the phrases that start in tile t (0 where entry[t] is LZ_NONE)
//   MODE 2  the phrases of tile t to ph_src / ph_len from slot offs[t] on, in position order
// The marks race benignly: a lane may see a mark another lane set in the same round, and then marks a position that is
// on the path as well (2^round steps behind a position of the path).
template <int MODE>
__global__ __launch_bounds__(LZ_NT) void lz_tile_kernel(const u64 *__restrict__ pack, u32 n, u32 ltile, u32 *__restrict__ exitp,
                                                        const u32 *__restrict__ entry, u64 *__restrict__ cnt,
                                                        const u64 *__restrict__ offs, const u8 *__restrict__ text,
                                                        u32 *__restrict__ ph_src, u32 *__restrict__ ph_len) {
    extern __shared__ __attribute__((aligned(16))) u32 lz_lds[];
    __shared__ u32 s_scan[LZ_NT / 64 + 1];
    const u32 tile = 1u << ltile, t = blockIdx.x, base = t << ltile;
    const u32 tlen = n - base < tile ? n - base : tile;
    u32 *a = lz_lds, *b = lz_lds + tile;
    u8 *mark = reinterpret_cast<u8 *>(lz_lds + 2 * tile);
    u32 e = 0;
    if (MODE) {
        e = entry[t];
        if (e == LZ_NONE || e < base || e - base >= tlen) {     // (uniform over the workgroup)
            if (MODE == 1 && threadIdx.x == 0) cnt[t] = 0;
            return;
        }
        e -= base;
    }
    for (u32 i = threadIdx.x; i < tlen; i += LZ_NT) {
        const u32 l = (u32)pack[base + i];
        a[i] = i + (l ? l : 1u);
        if (MODE) mark[i] = i == e ? 1 : 0;
    }
    __syncthreads();
    for (u32 round = 0; round < ltile; round++) {
        for (u32 i = threadIdx.x; i < tlen; i += LZ_NT) {
            const u32 v = a[i];
            if (MODE && v < tlen && mark[i]) mark[v] = 1;
            b[i] = v < tlen ? a[v] : v;
        }
        __syncthreads();
        u32 *const sw = a;
        a = b;
        b = sw;
    }
    if (MODE == 0) {
        for (u32 i = threadIdx.x; i < tlen; i += LZ_NT) exitp[base + i] = base + a[i];
        return;
    }
    // thread k owns the positions [k per, k per + per) of the tile
    const u32 per = tile >= LZ_NT ? tile / LZ_NT : 1u;
    const u32 lo = threadIdx.x * per;
    u32 c = 0;
    for (u32 k = lo; k < lo + per && k < tlen; k++) c += mark[k];
    u32 total;
    const u32 before = block_excl_sum<LZ_NT>(c, s_scan, &total);
    if (MODE == 1) {
        if (threadIdx.x == 0) cnt[t] = total;
        return;
    }
    u64 o = offs[t] + before;
    for (u32 k = lo; k < lo + per && k < tlen; k++) {
        if (!mark[k]) continue;
        const u64 v = pack[base + k];
        const u32 l = (u32)v;
        ph_len[o] = l;
        ph_src[o] = l ? (u32)(v >> 32) : (u32)text[base + k];
        o++;
    }
}

// step b: one lane follows exit from 0 (entry[] = LZ_NONE before the launch)
__global__ void lz_chain_kernel(const u32 *__restrict__ exitp, u32 n, u32 ltile, u32 *__restrict__ entry) {
    if (blockIdx.x || threadIdx.x) return;
    u32 pos = 0;
    while (pos < n) {
        entry[pos >> ltile] = pos;
        const u32 nx = exitp[pos];
        if (nx <= pos) break;                   // (an exit lies at or behind its tile's end: not reached)
        pos = nx;
    }
}

// ---- the inverse ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lz_un_len_kernel(const u32 *__restrict__ ph_len, u64 nph, u64 *__restrict__ len64) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nph) return;
    const u32 l = ph_len[p];
    len64[p] = l ? l : 1u;
}
// bad[0] = 1 for a list no parse is: a copy whose source is not strictly before its own start, a literal above 255
__global__ __launch_bounds__(256) void lz_un_check_kernel(const u32 *__restrict__ ph_src, const u32 *__restrict__ ph_len,
                                                          const u64 *__restrict__ starts, u64 nph, u32 *__restrict__ bad) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nph) return;
    if (ph_len[p] ? (u64)ph_src[p] >= starts[p] : ph_src[p] > 255u) bad[0] = 1u;
}
// one lane per output byte: its phrase by binary search over the starts (starts[0] = 0), then its parent; a literal's
// byte goes to out
__global__ __launch_bounds__(256) void lz_un_parent_kernel(const u32 *__restrict__ ph_src, const u32 *__restrict__ ph_len,
                                                           const u64 *__restrict__ starts, u64 nph, u32 total,
                                                           u32 *__restrict__ parent, u8 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    u64 lo = 0, hi = nph;                       // the last p with starts[p] <= i lies in [lo, hi)
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (starts[mid] <= i) lo = mid; else hi = mid;
    }
    if (ph_len[lo]) {
        parent[i] = ph_src[lo] + (u32)(i - starts[lo]);
    } else {
        parent[i] = (u32)i;
        out[i] = (u8)ph_src[lo];
    }
}
// one round: pb = pa o pa; *changed = 1 where that moved an entry
__global__ __launch_bounds__(256) void lz_un_jump_kernel(const u32 *__restrict__ pa, u32 *__restrict__ pb, u32 total,
                                                         u32 *__restrict__ changed) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u32 v = pa[i], w = pa[v];
    pb[i] = w;
    if (w != v) changed[0] = 1u;
}
// every copied byte from its root, a literal (roots are not written)
__global__ __launch_bounds__(256) void lz_un_gather_kernel(const u32 *__restrict__ parent, u32 total, u8 *out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u32 v = parent[i];
    if (v != i) out[i] = out[v];
}
#endif  // TC_FM_MS_HOST_CHECK
