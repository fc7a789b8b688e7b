// tc_fm_ms.hpp -- FM-index matching statistics and maximal exact matches (included by tc_fm_host.hpp, whose rank lines,
// tables and fm_mm_occ2 it uses).  No counterpart in the reference.  host/check/fm_ms_kernels.cpp
// compiles the same kernel bodies as plain C++ (TC_FM_MS_HOST_CHECK: the HIP keywords defined away, a workgroup of one
// lane, the lanes of a grid run one after another; the thread index, the barrier and the loads stand behind the small
// inline functions below).
//
// For a pattern p of length m and every 0 <= i < m: ms_len[i] = the largest l such that p[i .. i + l) occurs in the text
// (inside it, never over its end), ms_pos[i] = the first suffix-array row of that string's interval (sa[row] + 1 on a
// full index; fm_factor_walk_kernel turns rows into positions on a sampled one), ms_occ[i] = the interval's width.
//
// The loop is the single-symbol loop of fm_factor_kernel that, where a step comes back empty, does not close the phrase
// but SHRINKS it: [s, e] (1-based, inclusive; a = s - 1 and b = e - 1 the 0-based rows) is the interval of the match
// that starts at the position behind the current one, len its length.  For i = m - 1 down to 0, c = the code of p[i]:
//   1  c does not occur in the text: len = 0, done with i
//   2  len == 0: [s, e] = the table's interval of c, len = 1, done
//   3  one step with fm_mm_occ2 into (s2, e2), only while len < N - 1 (a match is at most the text); not empty and
//      e2 <= N: take it, len += 1, done
//   4  otherwise shrink to the parent interval: d = max(lcp[a], lcp[b + 1]) (0 for b + 1 = N), which is < len because
//      the rows around the interval of a string of length len share less than len bytes with it.  d = 0: len = 0, case 2.
//      Else a = the largest row <= a with lcp[row] < d, b = (the smallest row > b with lcp[row] < d) - 1 or N - 1,
//      len = d, case 3 again.
// Every string of depth in (d, len] has the interval [a, b] and so fails the same step: that is why the shrink may jump
// to d at once.  Termination: every step raises len by one and every shrink lowers it by at least one; len starts at 0,
// a position is done after one step or one opening, so a pattern takes at most 2 m + 1 turns of the inner loop.
//
// The two row searches go over a min tree of the LCP array with fan-out f (64; the debug interface builds 4, 8 or 16):
// level 0 is lcp itself, entry j of level k + 1 is the minimum of entries [f j, f j + f) of level k, up to the first
// level of at most f entries; every tree level starts at a multiple of 4 words of lmin.  A search scans the rest of its
// group of f entries with 16-byte loads; if no entry is below d it climbs -- the sibling minima of the next level, and
// so on -- and then descends into the nearest group whose minimum is below d: at most 2 f words per level and
// ceil(log_f N) levels on any text, so a unary or periodic text does not turn a shrink into a walk over the interval.
// The LCP part is never imported, so it is this library's own data; still the searches are bounded on any content:
// the downward one stops at group 0 of a level (row 0 at the latest, where lcp[0] = 0 ends it), the upward one at the
// end of a level (row N), no index at or above a level's entry count is used (a 16-byte load that straddles the count
// stays in the count's aligned 16 bytes and its surplus entries are masked), and a descent that finds nothing -- it
// cannot -- takes the group's first entry.
//
// Pair vectors are not used: a two-symbol step does not yield the interval -- and so not the first row -- of the
// position between the two symbols.  (A ms_len-only instance could take pair steps where they succeed: the follow-up.)
#pragma once

#define FM_MS_MAXLEV 20          // levels of the min tree, level 0 included: fan-out 4 over 2^31 rows has 16

#ifdef TC_FM_MS_HOST_CHECK
#include <stdint.h>
#include <string.h>
typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
#ifndef FM_LINE_BITS
#define FM_LINE_BITS 448
#endif
// ---- plain C++: one lane per workgroup; the launcher of host/check/fm_ms_kernels.cpp sets fm_ms_block
#define FM_MS_NT 1
#define FM_MS_KERNEL static void
#define FM_MS_SMALL_KERNEL static void
#define FM_MS_SEARCH static u32
#define FM_MS_DEVICE static inline
#define FM_MS_HD static inline
#define FM_MS_SHARED static
static u32 fm_ms_block = 0;
static u64 fm_ms_turns = 0;                                 // turns of the inner loop since the check reset it
static u64 fm_ms_climbed[2][FM_MS_MAXLEV + 1] = {};         // [0: downward, 1: upward][the highest level a search scanned]
#define FM_MS_TURN() (fm_ms_turns++)
#define FM_MS_CLIMBED(dir, lev) (fm_ms_climbed[dir][lev]++)
static inline u32 fm_ms_tid() { return 0; }
static inline u32 fm_ms_bid() { return fm_ms_block; }
static inline void fm_ms_sync() {}
static inline u32 fm_ms_clz(u32 x) { return (u32)__builtin_clz(x); }
static inline u32 fm_ms_ctz(u32 x) { return (u32)__builtin_ctz(x); }
struct FmMsQuad { u32 v[4]; };
// entries [i, i + 4) of a level of cnt entries, i a multiple of 4; the entries from cnt on read as 0xffffffff
static inline FmMsQuad fm_ms_load4(const u32 *lv, u32 i, u32 cnt) {
    FmMsQuad q;
    for (u32 k = 0; k < 4; k++) q.v[k] = i + k < cnt ? lv[i + k] : 0xffffffffu;
    return q;
}
static inline u32 fm_ms_load_word(const u8 *aligned) {
    u32 w;
    memcpy(&w, aligned, 4);
    return w;
}
// fm_mm_occ2 (csrc/tc_fm_mm.hpp) as a plain loop over the same 64-byte lines
static inline u32 fm_ms_rank_plain(const u64 *line, u32 off) {
    u32 r = (u32)line[0];
    for (u32 w = 0; w < 7; w++) {
        const u32 lo = w * 64;
        if (off >= lo + 64) r += (u32)__builtin_popcountll(line[1 + w]);
        else if (off > lo) r += (u32)__builtin_popcountll(line[1 + w] & ((1ull << (off - lo)) - 1ull));
    }
    return r;
}
static inline void fm_ms_occ2(const u64 *vec, u64 lines, u32 v, u32 k1, u32 k2, u32 *r1, u32 *r2) {
    const u32 l1 = k1 / FM_LINE_BITS, l2 = k2 / FM_LINE_BITS;
    *r1 = fm_ms_rank_plain(vec + ((u64)v * lines + l1) * 8, k1 - l1 * FM_LINE_BITS);
    *r2 = fm_ms_rank_plain(vec + ((u64)v * lines + l2) * 8, k2 - l2 * FM_LINE_BITS);
}
#else
#define FM_MS_NT 256
#define FM_MS_KERNEL __global__ __launch_bounds__(256, 8) void
#define FM_MS_SMALL_KERNEL __global__ __launch_bounds__(256) void
#define FM_MS_SEARCH __device__ __noinline__ u32
#define FM_MS_DEVICE __device__ __forceinline__
#define FM_MS_HD __host__ __device__ inline
#define FM_MS_SHARED __shared__
#define FM_MS_TURN() ((void)0)
#define FM_MS_CLIMBED(dir, lev) ((void)0)
FM_MS_DEVICE u32 fm_ms_tid() { return threadIdx.x; }
FM_MS_DEVICE u32 fm_ms_bid() { return blockIdx.x; }
FM_MS_DEVICE void fm_ms_sync() { __syncthreads(); }
FM_MS_DEVICE u32 fm_ms_clz(u32 x) { return (u32)__clz((int)x); }
FM_MS_DEVICE u32 fm_ms_ctz(u32 x) { return (u32)__builtin_ctz(x); }
struct FmMsQuad { u32 v[4]; };
// entries [i, i + 4) of a level of cnt entries, i a multiple of 4, as one 16-byte load (every level starts 16-byte
// aligned; the aligned 16 bytes that hold a valid entry lie in that entry's page); the entries from cnt on read as
// 0xffffffff
FM_MS_DEVICE FmMsQuad fm_ms_load4(const u32 *__restrict__ lv, u32 i, u32 cnt) {
    const uint4 t = *reinterpret_cast<const uint4 *>(lv + i);
    FmMsQuad q;
    q.v[0] = t.x;
    q.v[1] = i + 1 < cnt ? t.y : 0xffffffffu;
    q.v[2] = i + 2 < cnt ? t.z : 0xffffffffu;
    q.v[3] = i + 3 < cnt ? t.w : 0xffffffffu;
    return q;
}
FM_MS_DEVICE u32 fm_ms_load_word(const u8 *aligned) { return *reinterpret_cast<const u32 *>(aligned); }
FM_MS_DEVICE void fm_ms_occ2(const u64 *__restrict__ vec, u64 lines, u32 v, u32 k1, u32 k2, u32 *r1, u32 *r2) {
    fm_mm_occ2(vec, lines, v, k1, k2, r1, r2);
}
#endif

// The shape of the min tree over N rows at fan-out 2^lf, the same for the build, the queries and the device-bytes
// report: off[k] / cnt[k] = the first word in lmin and the entry count of level k (off[0] is unused: level 0 is lcp,
// cnt[0] = N), k = 1 .. the returned number of tree levels (at least 1; the last has at most 2^lf entries); *words = the
// words of lmin, every level rounded up to a multiple of 4.
FM_MS_HD u32 fm_ms_tree_shape(u32 N, u32 lf, u32 *off, u32 *cnt, u32 *words) {
    u32 lev = 0, cur = N, at = 0;
    off[0] = 0;
    cnt[0] = N;
    do {
        cur = (u32)(((u64)cur + (1u << lf) - 1u) >> lf);
        lev++;
        off[lev] = at;
        cnt[lev] = cur;
        at += (cur + 3u) & ~3u;
    } while (cur > (1u << lf) && lev + 1 < FM_MS_MAXLEV);
    *words = at;
    return lev;
}

// one level of the tree: dst[j] = the minimum of src[f j .. min(f j + f, src_cnt)), j < dst_cnt; the words up to the
// level's multiple of 4 are set to 0xffffffff
FM_MS_SMALL_KERNEL fm_lmin_kernel(const u32 *__restrict__ src, u32 src_cnt, u32 lf, u32 *__restrict__ dst, u32 dst_cnt) {
    const u32 j = fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (j >= ((dst_cnt + 3u) & ~3u)) return;
    u32 m = 0xffffffffu;
    if (j < dst_cnt) {
        const u32 lo = j << lf;
        for (u32 c = lo; c < lo + (1u << lf) && c < src_cnt; c += 4) {
            const FmMsQuad q = fm_ms_load4(src, c, src_cnt);
            for (int k = 0; k < 4; k++) m = q.v[k] < m ? q.v[k] : m;
        }
    }
    dst[j] = m;
}

// what the searches know of the tree (s_off / s_cnt: fm_ms_tree_shape, in LDS)
struct FmMsTree {
    const u32 *lcp, *lmin, *s_off, *s_cnt;
    u32 nlev, lf;
};
FM_MS_DEVICE const u32 *fm_ms_level(const FmMsTree &T, u32 lev) { return lev ? T.lmin + T.s_off[lev] : T.lcp; }

// the largest row <= a with lcp[row] < d (d >= 1, so row 0 qualifies)
FM_MS_SEARCH fm_ms_prev_below(const FmMsTree T, u32 a, u32 d) {
    const u32 fmask = (1u << T.lf) - 1u;
    u32 pos = a, lev = 0;
    while (true) {              // climb: the entries of pos's group at or before pos, last first
        const u32 *lv = fm_ms_level(T, lev);
        const u32 cnt = T.s_cnt[lev], g0 = pos & ~fmask;
        u32 found = 0xffffffffu;
        for (u32 c = pos & ~3u;; c -= 4) {
            const FmMsQuad q = fm_ms_load4(lv, c, cnt);
            u32 m = 0;
            for (u32 k = 0; k < 4; k++) m |= (q.v[k] < d && c + k <= pos) ? 1u << k : 0u;
            if (m) {
                found = c + 31u - fm_ms_clz(m);
                break;
            }
            if (c == g0) break;
        }
        if (found != 0xffffffffu) {
            pos = found;
            break;
        }
        if (g0 == 0 || lev == T.nlev) return 0;     // (entry 0 of every level is lcp[0] = 0: not reached)
        pos = (pos >> T.lf) - 1u;
        lev++;
    }
    FM_MS_CLIMBED(0, lev);
    while (lev) {               // descend: the last child below d
        lev--;
        const u32 *lv = fm_ms_level(T, lev);
        const u32 cnt = T.s_cnt[lev], lo = pos << T.lf;
        const u32 hi = lo + fmask < cnt - 1u ? lo + fmask : cnt - 1u;
        pos = lo;
        for (u32 c = hi & ~3u;; c -= 4) {
            const FmMsQuad q = fm_ms_load4(lv, c, cnt);
            u32 m = 0;
            for (u32 k = 0; k < 4; k++) m |= (q.v[k] < d && c + k <= hi) ? 1u << k : 0u;
            if (m) {
                pos = c + 31u - fm_ms_clz(m);
                break;
            }
            if (c == lo) break;
        }
    }
    return pos;
}

// the smallest row > b with lcp[row] < d, or N when there is none
FM_MS_SEARCH fm_ms_next_below(const FmMsTree T, u32 N, u32 b, u32 d) {
    const u32 fmask = (1u << T.lf) - 1u;
    u32 pos = b + 1u, lev = 0;
    while (true) {              // climb: the entries of pos's group from pos on, first first
        if (lev > T.nlev) return N;
        const u32 cnt = T.s_cnt[lev];
        if (pos >= cnt) return N;
        const u32 *lv = fm_ms_level(T, lev);
        const u32 gl = (pos | fmask) < cnt - 1u ? (pos | fmask) : cnt - 1u;
        u32 found = 0xffffffffu;
        for (u32 c = pos & ~3u; c <= gl; c += 4) {
            const FmMsQuad q = fm_ms_load4(lv, c, cnt);
            u32 m = 0;
            for (u32 k = 0; k < 4; k++) m |= (q.v[k] < d && c + k >= pos) ? 1u << k : 0u;
            if (m) {
                found = c + fm_ms_ctz(m);
                break;
            }
        }
        if (found != 0xffffffffu) {
            pos = found;
            break;
        }
        pos = (pos >> T.lf) + 1u;
        lev++;
    }
    FM_MS_CLIMBED(1, lev);
    while (lev) {               // descend: the first child below d
        lev--;
        const u32 *lv = fm_ms_level(T, lev);
        const u32 cnt = T.s_cnt[lev], lo = pos << T.lf;
        const u32 hi = lo + fmask < cnt - 1u ? lo + fmask : cnt - 1u;
        pos = lo;
        for (u32 c = lo; c <= hi; c += 4) {
            const FmMsQuad q = fm_ms_load4(lv, c, cnt);
            u32 m = 0;
            for (u32 k = 0; k < 4; k++) m |= (q.v[k] < d) ? 1u << k : 0u;
            if (m) {
                pos = c + fm_ms_ctz(m);
                break;
            }
        }
    }
    return pos;
}

// One lane per pattern.  POS = false writes ms_len alone; POS = true also ms_pos and ms_occ, each where it is not null
// (sa = null: a sampled index, ms_pos receives rows).  Results of pattern p go to [offs[p], offs[p + 1]) of the arrays.
template <bool POS>
FM_MS_KERNEL fm_ms_kernel(const u64 *__restrict__ bits, u64 lines, const u32 *__restrict__ tab, u32 N,
                          const u32 *__restrict__ lcp, const u32 *__restrict__ lmin, u32 lf, const u32 *__restrict__ sa,
                          const u8 *__restrict__ pats, const u64 *__restrict__ offs, u64 npat, u32 *__restrict__ ms_len,
                          u64 *__restrict__ ms_pos, u32 *__restrict__ ms_occ) {
    FM_MS_SHARED u32 s_tab[768];
    FM_MS_SHARED u32 s_off[FM_MS_MAXLEV + 1], s_cnt[FM_MS_MAXLEV + 1], s_nlev;
    for (u32 i = fm_ms_tid(); i < 768; i += FM_MS_NT) s_tab[i] = tab[i];
    if (fm_ms_tid() == 0) {
        u32 words;
        s_nlev = fm_ms_tree_shape(N, lf, s_off, s_cnt, &words);
    }
    fm_ms_sync();
    const u64 p = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (p >= npat) return;
    const u64 beg = offs[p];
    const u8 *const pp = pats + beg;            // pp[j] = p[j]
    u64 q = offs[p + 1] - beg;                  // positions still to be answered: the next one is q - 1
    FmMsTree T;
    T.lcp = lcp; T.lmin = lmin; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    // the pattern is read right to left through the aligned 4-byte window of fm_factor_kernel (the aligned word that
    // holds a valid byte lies in that byte's page, so reading it whole is always safe)
    u32 widx = 0, word = 0;
    auto load_window = [&](const u8 *ad) {
        widx = (u32)((uintptr_t)ad >> 2);
        word = fm_ms_load_word(reinterpret_cast<const u8 *>((uintptr_t)ad & ~(uintptr_t)3));
    };
    auto byte_at = [&](u64 j) -> u32 {          // pp[j]
        const u8 *ad = pp + j;
        if ((u32)((uintptr_t)ad >> 2) != widx) load_window(ad);
        return (word >> (8 * ((u32)(uintptr_t)ad & 3u))) & 255u;
    };
    if (q) load_window(pp + q - 1);
    u32 s = 0, e = 0, len = 0;
    while (q != 0) {
        const u32 c = s_tab[byte_at(q - 1)];
        if (c == 0xFFFFFFFFu) {
            len = 0;                            // case 1
        } else {
            while (true) {
                FM_MS_TURN();
                if (len == 0) {                 // case 2 (an interval that leaves [1, N] -- not on an index of this library -- stays closed)
                    const u32 s2 = s_tab[256 + c] + 1u, e2 = s_tab[256 + c] + s_tab[512 + c];
                    if (s2 <= e2 && e2 <= N) {
                        s = s2;
                        e = e2;
                        len = 1;
                    }
                    break;
                }
                if (len < N - 1u) {             // case 3
                    u32 o1, o2;
                    fm_ms_occ2(bits, lines, c, s - 1u, e, &o1, &o2);
                    const u64 s2 = (u64)s_tab[256 + c] + o1 + 1u, e2 = (u64)s_tab[256 + c] + o2;
                    if (s2 <= e2 && e2 <= (u64)N) {
                        s = (u32)s2;
                        e = (u32)e2;
                        len++;
                        break;
                    }
                }
                const u32 la = lcp[s - 1u], lb = e < N ? lcp[e] : 0u;      // case 4 (rows a = s - 1 and b + 1 = e)
                u32 d = la > lb ? la : lb;
                if (d >= len) d = len - 1u;     // (d < len on an LCP array of this text: keeps the loop finite on any content)
                len = d;
                if (d == 0) continue;
                s = fm_ms_prev_below(T, s - 1u, d) + 1u;
                e = fm_ms_next_below(T, N, e - 1u, d);
            }
        }
        q--;
        const u64 o = beg + q;
        ms_len[o] = len;
        if (POS) {
            if (ms_pos) ms_pos[o] = len ? (sa ? (u64)sa[s - 1u] + 1u : (u64)(s - 1u)) : 0u;
            if (ms_occ) ms_occ[o] = len ? e - s + 1u : 0u;
        }
    }
}

// ---- maximal exact matches: the positions of a pattern whose match is at least min_len long and is not the tail of
// the match one position to the left (ms_len[i - 1] <= ms_len[i]; ms_len[i - 1] <= ms_len[i] + 1 always holds).
// One lane per pattern, twice: cnt[p] = its MEMs; then, behind the scan of the counts, its segment [moffs[p],
// moffs[p + 1]) in increasing i, no atomics: mem_start = i, mem_pos = ms_pos[i] (a row on a sampled index: the walk over
// the MEM list follows), mem_len = ms_len[i].
FM_MS_DEVICE bool fm_mem_is(const u32 *__restrict__ ms_len, u64 beg, u64 i, u32 min_len) {
    const u32 l = ms_len[beg + i];
    return l >= min_len && (i == 0 || ms_len[beg + i - 1] <= l);
}
FM_MS_SMALL_KERNEL fm_mem_count_kernel(const u32 *__restrict__ ms_len, const u64 *__restrict__ offs, u64 npat, u32 min_len,
                                       i64 *__restrict__ cnt) {
    const u64 p = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (p >= npat) return;
    const u64 beg = offs[p], m = offs[p + 1] - beg;
    u64 k = 0;
    for (u64 i = 0; i < m; i++) k += fm_mem_is(ms_len, beg, i, min_len) ? 1u : 0u;
    cnt[p] = (i64)k;
}
FM_MS_SMALL_KERNEL fm_mem_fill_kernel(const u32 *__restrict__ ms_len, const u64 *__restrict__ ms_pos,
                                      const u64 *__restrict__ offs, u64 npat, u32 min_len, const u64 *__restrict__ moffs,
                                      u64 *__restrict__ mem_start, u64 *__restrict__ mem_pos, u32 *__restrict__ mem_len) {
    const u64 p = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (p >= npat) return;
    const u64 beg = offs[p], m = offs[p + 1] - beg, hi = moffs[p + 1];
    u64 o = moffs[p];
    for (u64 i = 0; i < m && o < hi; i++) {
        if (!fm_mem_is(ms_len, beg, i, min_len)) continue;
        mem_start[o] = i;
        mem_pos[o] = ms_pos[beg + i];
        mem_len[o] = ms_len[beg + i];
        o++;
    }
}
