// tc_rep.hpp -- the maximal and supermaximal repeats of a text from its enhanced suffix array (included by
// tc_rep_host.hpp behind tc_fm_host.hpp, whose min tree and row searches -- tc_fm_ms.hpp -- it uses unchanged; DESIGN.md
// section 4.7).  No counterpart in the reference.  host/check/rep_kernels.cpp compiles rep_row_kernel as plain C++
// (TC_FM_MS_HOST_CHECK, as tc_fm_ms.hpp describes); the flag, count and fill kernels are streaming passes with a
// workgroup scan and exist on the device only.
//
// N = n + 1 rows, sa / lcp as tc_lcp_array defines them, left(r) = text[sa[r] - 1], Nothing (which differs from every
// byte) for the row `primary` with sa = 0: that is the last column sa_build writes (L[primary] = 0 by convention).
// A repeat w of length l >= 1 is an LCP interval [lb, rb], lb < rb: l = min lcp[lb + 1 .. rb], lcp[lb] < l, and
// rb = N - 1 or lcp[rb + 1] < l.  It is
//   maximal       iff left(lb .. rb) are not all equal (right-maximal is what being an LCP interval means);
//   supermaximal  iff lcp[k] = l for every k in lb + 1 .. rb (no child interval) and left(lb .. rb) are pairwise
//                 distinct: at most 256 bytes and one Nothing, so occ <= 257.
// Every interval is reported once, from its REPRESENTATIVE ROW j = the smallest row in (lb, rb] with lcp[j] = l, and the
// output is in increasing j.  That order is deterministic, and for equal lb it is decreasing len (a child that shares its
// parent's lb has the smaller representative), but it is NOT sorted by lb.  "aaabaab" has
//   sa   7  0  4  1  5  2  6  3          lcp  0  0  2  3  1  2  0  1
// and the three maximal repeats [1, 3] of "aa" (j = 2), [2, 3] of "aab" (j = 3) and [1, 5] of "a" (j = 4): the rows come
// out as 1, 2, 1 with the lengths 2, 3, 1 -- the parent [1, 5] behind both its child and its grandchild, because its own
// depth shows first at row 4.
//
// No lane walks the LCP array.  chg[k] = the number of rows r in 1 .. k with left(r) != left(r - 1) (the primary row
// differs from both its neighbours): rep_left_kernel writes the flags, tc_scan64 sums them, and left is not all equal on
// [lb, rb] iff chg[rb] - chg[lb] > 0, pairwise distinct only if chg[rb] - chg[lb] = rb - lb.  Then one lane per row j:
//   l = lcp[j]; l < min_len: none, before any search
//   lb = the largest row <= j - 1 with lcp < l                           (fm_ms_prev_below)
//   j is the representative iff the largest row <= j - 1 with lcp < l + 1 is lb as well   (lb = j - 1: it is, no search)
//   rb = (the smallest row > j with lcp < l, or N) - 1                   (fm_ms_next_below)
// so at most three searches of at most 2 f words per level.  The result is one packed 8-byte word per row,
// occ << 32 | lb (occ = 0: none), which the count and the fill pass both stream: the searches run once.
#pragma once
#ifdef TC_FM_MS_HOST_CHECK
#include "tc_fm_ms.hpp"
#endif

#define REP_NT 256
#define REP_ITEMS 4
#define REP_TILE (REP_NT * REP_ITEMS)   // rows per tile of the count and fill passes
#define REP_MAX_SUPER_OCC 257u          // 256 bytes and Nothing

// One lane per suffix-array row j.  lmin: the min tree (fm_lmin_kernel, fan-out 2^lf) over lcp; chg, L: N entries each.
// SUPER = false: the maximal repeats; true: the supermaximal ones (a supermaximal interval has no child, so its
// representative is lb + 1 and no second search is needed).  The 256 left bytes seen are four u64 updated by selects: an
// array indexed by the byte would go to scratch.
template <bool SUPER>
FM_MS_KERNEL rep_row_kernel(const u32 *__restrict__ lcp, const u32 *__restrict__ lmin, u32 N, u32 lf,
                            const u64 *__restrict__ chg, const u8 *__restrict__ L, u32 primary, u32 min_len, u32 min_occ,
                            u64 *__restrict__ pack) {
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 j64 = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (j64 >= N) return;
    const u32 j = (u32)j64, l = lcp[j];
    if (j == 0 || l == 0 || l < min_len) {      // (the searches need d >= 1)
        pack[j] = 0;
        return;
    }
    FmMsTree T;
    T.lcp = lcp; T.lmin = lmin; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    const u32 lb = fm_ms_prev_below(T, j - 1u, l);
    u64 out = 0;
    if (lb == j - 1u || (!SUPER && fm_ms_prev_below(T, j - 1u, l + 1u) == lb)) {
        const u32 rb = fm_ms_next_below(T, N, j, l) - 1u;
        const u32 occ = rb - lb + 1u;
        const u64 changes = chg[rb] - chg[lb];
        bool ok = occ >= min_occ;
        if (!SUPER) {
            ok = ok && changes != 0;
        } else {
            ok = ok && occ <= REP_MAX_SUPER_OCC && changes == (u64)(occ - 1u);
            if (ok) {
                u64 b0 = 0, b1 = 0, b2 = 0, b3 = 0;
                for (u32 k = lb; k <= rb; k++) {
                    if (k > lb && lcp[k] != l) ok = false;
                    if (k == primary) continue;         // Nothing: there is one, and it differs from every byte
                    const u32 c = L[k], w = c >> 6;
                    const u64 bit = 1ull << (c & 63u);
                    const u64 cur = w == 0 ? b0 : w == 1 ? b1 : w == 2 ? b2 : b3;
                    if (cur & bit) ok = false;
                    b0 |= w == 0 ? bit : 0ull;
                    b1 |= w == 1 ? bit : 0ull;
                    b2 |= w == 2 ? bit : 0ull;
                    b3 |= w == 3 ? bit : 0ull;
                }
            }
        }
        if (ok) out = (u64)occ << 32 | lb;
    }
    pack[j] = out;
}

#ifndef TC_FM_MS_HOST_CHECK
// flag[r] = 1 where left(r + 1) != left(r), r + 1 < N (flag[N - 1] = 0): the exclusive scan of the flags is chg itself,
// chg[k] = the flags of the rows 0 .. k - 1 = the changes at the rows 1 .. k
__global__ __launch_bounds__(256) void rep_left_kernel(const u8 *__restrict__ L, u32 N, u32 primary, u64 *__restrict__ flag) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    flag[r] = r + 1 < N && (r == primary || r + 1 == primary || L[r + 1] != L[r]) ? 1u : 0u;
}

// cnt[t] = the repeats whose representative row lies in tile t
__global__ __launch_bounds__(REP_NT) void rep_count_kernel(const u64 *__restrict__ pack, u32 N, u64 *__restrict__ cnt) {
    __shared__ u32 s[REP_NT / 64];
    const u64 base = (u64)blockIdx.x * REP_TILE;
    u32 c = 0;
    for (u32 k = 0; k < REP_ITEMS; k++) {
        const u64 j = base + (u64)k * REP_NT + threadIdx.x;
        if (j < N) c += (pack[j] >> 32) ? 1u : 0u;
    }
    c = wave_sum(c);
    if (lane_id() == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 tot = 0;
        for (u32 w = 0; w < REP_NT / 64; w++) tot += s[w];
        cnt[blockIdx.x] = tot;
    }
}

// the repeats of tile t to the four arrays from slot offs[t] on, in row order: lane k owns the rows
// [k REP_ITEMS, k REP_ITEMS + REP_ITEMS) of the tile, a workgroup scan gives its first slot.  rep_row may be null.
__global__ __launch_bounds__(REP_NT) void rep_fill_kernel(const u64 *__restrict__ pack, u32 N, const u64 *__restrict__ offs,
                                                          const u32 *__restrict__ sa, const u32 *__restrict__ lcp,
                                                          u32 *__restrict__ rep_pos, u32 *__restrict__ rep_len,
                                                          u32 *__restrict__ rep_occ, u32 *__restrict__ rep_row) {
    __shared__ u32 s_scan[REP_NT / 64 + 1];
    const u64 base = (u64)blockIdx.x * REP_TILE + (u64)threadIdx.x * REP_ITEMS;
    u64 v[REP_ITEMS];
    u32 c = 0;
    for (u32 k = 0; k < REP_ITEMS; k++) {
        v[k] = base + k < N ? pack[base + k] : 0ull;
        c += (v[k] >> 32) ? 1u : 0u;
    }
    u32 total;
    const u32 before = block_excl_sum<REP_NT>(c, s_scan, &total);
    u64 o = offs[blockIdx.x] + before;
    for (u32 k = 0; k < REP_ITEMS; k++) {
        const u32 occ = (u32)(v[k] >> 32), lb = (u32)v[k];
        if (!occ) continue;
        rep_pos[o] = sa[lb];
        rep_len[o] = lcp[base + k];
        rep_occ[o] = occ;
        if (rep_row) rep_row[o] = lb;
        o++;
    }
}
#endif  // TC_FM_MS_HOST_CHECK
