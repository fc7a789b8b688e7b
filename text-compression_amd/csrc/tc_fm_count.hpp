// tc_fm_count.hpp -- the rank lookups of the FM-index and the backward search of one pattern (included by
// tc_fm_host.hpp; fm_count_kernel there is the launch around fm_count_lane).  host/check/fm_count_kernels.cpp compiles
// the same bodies as plain C++ (TC_FM_COUNT_HOST_CHECK: the HIP keywords defined away; the 16-byte loads, the popcount and
// the pattern window's load stand behind the small definitions below).
//
// What it reads.  The index may be an imported byte string (tc_fm_import_dev), i.e. caller data whose rank counts are
// arbitrary: a line's ones-before word is any 64-bit value.  An interval [s, e] (1-based, inclusive) is only ever stepped
// from, reported or written as a range when 1 <= s <= e <= N -- a step whose result is not of that shape ends the search
// with the answer 0 and no range, as an empty interval always did -- so the positions s - 1 < e <= N handed to fm_occ2
// lie in lines <= N / 448 < lines of the vector of a code < sigma (or of a pair < sigma^2: both codes come from the table,
// which holds codes below the number of present byte values only); table entries are indexed by a byte, by such a code or
// by such a pair; and the rows a locate copies out of the suffix array are s - 1 .. e - 1 < N.  The interval arithmetic is
// unsigned 64-bit: it wraps where the counts are absurd, and the shape test sees the wrapped value.  On an index this
// library built s <= e implies 1 <= s and e <= N, so no step is cut short and no answer changes.
#pragma once

#ifdef TC_FM_COUNT_HOST_CHECK
#include <stdint.h>
#include <string.h>
typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
#ifndef FM_LINE_BITS
#define FM_LINE_BITS 448
#endif
#define FM_CNT_DEVICE static inline
#define FM_CNT_UNROLL
struct __attribute__((may_alias)) FmWord2 { u64 x, y; };   // 16 bytes of a line
static inline u32 fm_cnt_popc(u64 v) { return (u32)__builtin_popcountll(v); }
static inline u64 fm_cnt_load8(uintptr_t aligned) {
    u64 w;
    memcpy(&w, reinterpret_cast<const void *>(aligned), 8);
    return w;
}
#else
#define FM_CNT_DEVICE __device__ __forceinline__
#define FM_CNT_UNROLL _Pragma("unroll")
typedef ulonglong2 FmWord2;
FM_CNT_DEVICE u32 fm_cnt_popc(u64 v) { return (u32)__popcll(v); }
FM_CNT_DEVICE u64 fm_cnt_load8(uintptr_t aligned) { return *reinterpret_cast<const u64 *>(aligned); }
#endif

// Occ(c, k): occurrences of code c in L[0 .. k)
FM_CNT_DEVICE u64 fm_occ(const u64 *__restrict__ bits, u64 lines, u32 c, u64 k) {
    u64 line = k / FM_LINE_BITS;
    u32 off = (u32)(k - line * FM_LINE_BITS);
    const FmWord2 *p = reinterpret_cast<const FmWord2 *>(bits + ((u64)c * lines + line) * 8);
    FmWord2 a = p[0], b = p[1], cc = p[2], d = p[3];
    u64 w[7] = {a.y, b.x, b.y, cc.x, cc.y, d.x, d.y};
    u64 r = a.x;
    u32 full = off >> 6, rem = off & 63;
    FM_CNT_UNROLL
    for (int i = 0; i < 7; i++) {
        u64 m = ((u32)i < full) ? ~0ull : (((u32)i == full) ? ((1ull << rem) - 1ull) : 0ull);
        r += (u64)fm_cnt_popc(w[i] & m);
    }
    return r;
}

// Occ(c, k1) and Occ(c, k2), k1 <= k2, of one backward-search step.  Once the range [s, e] has
// narrowed (after ~13 steps on a 2^28 DNA text it is a single row) both positions lie in the same
// 64-byte line: it is fetched once.  Lanes whose positions straddle two lines fetch the second one.
FM_CNT_DEVICE void fm_occ2(const u64 *__restrict__ bits, u64 lines, u32 c, u64 k1, u64 k2,
                           u64 *r1, u64 *r2) {
    const u64 line1 = k1 / FM_LINE_BITS, line2 = k2 / FM_LINE_BITS;
    const u32 off1 = (u32)(k1 - line1 * FM_LINE_BITS), off2 = (u32)(k2 - line2 * FM_LINE_BITS);
    const FmWord2 *p = reinterpret_cast<const FmWord2 *>(bits + ((u64)c * lines + line1) * 8);
    FmWord2 a = p[0], b = p[1], cc = p[2], d = p[3];
    {
        const u64 w[7] = {a.y, b.x, b.y, cc.x, cc.y, d.x, d.y};
        u64 r = a.x;
        const u32 full = off1 >> 6, rem = off1 & 63;
        FM_CNT_UNROLL
        for (int i = 0; i < 7; i++) {
            const u64 m = ((u32)i < full) ? ~0ull : (((u32)i == full) ? ((1ull << rem) - 1ull) : 0ull);
            r += (u64)fm_cnt_popc(w[i] & m);
        }
        *r1 = r;
    }
    if (line2 != line1) {
        const FmWord2 *q = reinterpret_cast<const FmWord2 *>(bits + ((u64)c * lines + line2) * 8);
        a = q[0]; b = q[1]; cc = q[2]; d = q[3];
    }
    {
        const u64 w[7] = {a.y, b.x, b.y, cc.x, cc.y, d.x, d.y};
        u64 r = a.x;
        const u32 full = off2 >> 6, rem = off2 & 63;
        FM_CNT_UNROLL
        for (int i = 0; i < 7; i++) {
            const u64 m = ((u32)i < full) ? ~0ull : (((u32)i == full) ? ((1ull << rem) - 1ull) : 0ull);
            r += (u64)fm_cnt_popc(w[i] & m);
        }
        *r2 = r;
    }
}

// an interval a step may be taken from, and the only kind that is reported: 1 <= s <= e <= N
FM_CNT_DEVICE bool fm_interval_ok(u64 s, u64 e, u64 N) { return s - 1 < e && e <= N; }

// countFMIndex (FMIndex/Internal.hs:347-438) of the pattern pats[beg .. end): the number of its occurrences, 0 for none,
// and for a non-empty result its interval in *rs, *re (1-based, inclusive; untouched otherwise).  s_tab = [0..255] code
// of byte (0xFFFFFFFF absent), [256..511] C[code], [512..767] cnt[code]; s_tab2 = C2[pair] (PAIRS only).
template <bool PAIRS>
FM_CNT_DEVICE i64 fm_count_lane(const u64 *__restrict__ bits, const u64 *__restrict__ bits2, u64 lines,
                                const u32 *s_tab, const u32 *s_tab2, u32 sigma, u64 N,
                                const u8 *__restrict__ pats, u64 beg, u64 end, u64 *rs, u64 *re) {
    u64 s = 1, e = N;                   // the whole index: what the first symbol's table interval replaces
    bool first = true, flag = false;
    // the pattern is read right to left through an aligned 8-byte window: one load per 8 steps instead of
    // one uncoalesced byte load per step (64 lanes = 64 different lines every time).  The aligned word
    // that holds a valid byte lies in that byte's page, so reading it whole is always safe.
    uintptr_t wbase = ~(uintptr_t)0;
    u64 word = 0;
    auto byte_at = [&](u64 q) -> u32 {   // pats[q]
        const uintptr_t ad = (uintptr_t)(pats + q);
        if ((ad & ~(uintptr_t)7) != wbase) {
            wbase = ad & ~(uintptr_t)7;
            word = fm_cnt_load8(wbase);
        }
        return (u32)(word >> (8 * (ad & 7))) & 255u;
    };
    u64 q = end;
    while (q > beg) {                   // right to left (:375)
        if (!fm_interval_ok(s, e, N)) { // :387-389 (s > e), and the shape every step relies on
            flag = true;
            break;
        }
        const u32 c = s_tab[byte_at(q - 1)];
        if (c == 0xFFFFFFFFu) break;    // findIndexL = Nothing: the loop just stops (:393,:421)
        const u64 C = (u64)s_tab[256 + c];
        if (first) {                    // :391-418
            s = C + 1;
            e = C + (u64)s_tab[512 + c];
            first = false;
            q--;
            continue;
        }
        if (PAIRS && q - 1 > beg) {     // two symbols by one lookup, when the one to the left occurs in the text too
            const u32 a = s_tab[byte_at(q - 2)];
            if (a != 0xFFFFFFFFu) {
                const u32 pr = a * sigma + c;
                u64 o1, o2;
                fm_occ2(bits2, lines, pr, s - 1, e, &o1, &o2);
                const u64 C2 = (u64)s_tab2[pr];
                s = C2 + o1 + 1;
                e = C2 + o2;
                q -= 2;
                continue;
            }
        }
        u64 o1, o2;                     // :424-432 (1 <= s <= e <= N here: s - 1 < e)
        fm_occ2(bits, lines, c, s - 1, e, &o1, &o2);
        s = C + o1 + 1;
        e = C + o2;
        q--;
    }
    if (first || flag || !fm_interval_ok(s, e, N)) return 0;  // :366-371
    *rs = s;
    *re = e;
    return (i64)(e - s + 1);
}
