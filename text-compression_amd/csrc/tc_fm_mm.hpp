// tc_fm_mm.hpp -- FM-index search with mismatches: count and locate within Hamming distance k (included by
// tc_fm_host.hpp, whose rank lines, tables and fm_occ2 it uses).  No counterpart in the reference.
//
// For a pattern p of length m the answer is every text position i, 0 <= i <= n - m, with Hamming(T[i .. i + m), p) <= k:
// substitutions only.  The search is a bounded depth-first enumeration over backward-search intervals: the strings v with
// Hamming(v, p) <= k that occur in the text ("variants") are visited one by one, each variant owns the suffix-array
// interval of the suffixes that begin with it, distinct variants have disjoint intervals, and a variant is a path from
// the pattern's end to its start on which at most k symbols were substituted -- so every hit is reported exactly once.
// Substitutes are drawn from the byte values of the text (codes 0 .. sigma - 1): a window of the text holds nothing
// else, so a pattern byte that does not occur in the text can only be a mismatch.  (fm_count_kernel stops its loop at
// such a byte, as the reference does; this kernel does not share that quirk.)
//
// Frames.  A frame is {q, s, e, alt}: q symbols of the pattern are still to be consumed (the next one is p[q - 1]),
// [s, e] is the interval (1-based, inclusive, as in fm_count_kernel) before consuming it, and alt is the next substitute
// code to try there.  A frame at depth d has spent d mismatches.  At the top frame:
//   q = 0                 report [s, e] with distance d, pop
//   d < k, alt < sigma    a = alt++; unless a is the pattern's own code: one step with a; a non-empty result pushes
//                         {q - 1, s', e', 0} (depth d + 1)
//   otherwise             the exact step with the pattern's own code (a byte without a code: pop), then q - 1, alt = 0
//                         in the same frame; an empty result pops
// The top frame lives in registers; the frames below it -- at most k = TC_FM_MAX_MISMATCH of them, not one per pattern
// position -- live in LDS (256 lanes x 3 frames x 16 bytes = 12 KB per workgroup: a dynamically indexed register array
// would go to scratch).  N < 2^32 (the suffix array is u32), so a frame is four u32.
// Once the budget is spent (d = k) the rest of the pattern is an exact tail, and with pair vectors it is the loop of
// fm_count_kernel<true>: two symbols per lookup where both occur in the text.  Pair steps are not taken while branches
// remain (d < k): every position must be offered its substitutes.
//
// Termination.  Every turn of the loop either advances alt (bounded by sigma), decrements q (bounded by m) or pops, and a
// push happens only at d < k, so the depth never exceeds k + 1 frames: the loop ends on any index content and any
// pattern.  What it reads.  The index may be an imported byte string, i.e. caller data whose rank counts are arbitrary.
// An interval is only ever stepped from when 1 <= s <= e <= N -- a step whose result is not of that shape counts as
// empty -- so the positions s - 1 < e <= N handed to fm_mm_occ2 lie in lines <= N / 448 < lines of the vector of a code
// < sigma (or of a pair < sigma^2); table entries are indexed by a byte, by such a code or by such a pair; and the rows
// written or looked up in the suffix array are s - 1 .. e - 1 < N.  On an index this library built no step is cut short.
//
// FILL = false sums the widths of the reported intervals into out[p].  FILL = true repeats the identical enumeration and
// writes into the pattern's own segment [hoffs[p], hoffs[p + 1]) of hits (and of hit_mm, when given): sa[row] + 1 on a
// full index, the row itself on a sampled one (sa = null; fm_locate_walk_kernel then turns rows into positions).  No
// atomics: a lane writes its segment front to back, which is what makes the order deterministic.  An interval is
// written lane-serially whatever its width -- reports happen where the lanes of a wave have diverged, so the
// wave-cooperative copy of fm_locate_fill_kernel has no convergent point to run at; with k >= 1 nearly every reported
// interval of a pattern longer than log_sigma n is a single row.
#pragma once

#define FM_MM_MAXK 3   // = TC_FM_MAX_MISMATCH (textcomp.h; static_assert in tc_fm_host.hpp)

// fm_occ2 in 32-bit arithmetic: Occ(v, k1) and Occ(v, k2), k1 <= k2 <= N < 2^32, from one line where both positions share
// it.  Counts below 2^32 need only the low half of a line's ones-before word, and the payload is taken as 14 words of 32
// bits, so masks and sums are one register each: this is what keeps the enumeration at 64 VGPRs.
__device__ __forceinline__ u32 fm_mm_rank(const ulonglong2 a, const ulonglong2 b, const ulonglong2 cc, const ulonglong2 d,
                                          u32 off) {
    const u64 w[7] = {a.y, b.x, b.y, cc.x, cc.y, d.x, d.y};
    u32 r = (u32)a.x;
    const u32 full = off >> 5, rem = off & 31;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        const u32 h = (u32)(w[i >> 1] >> (32 * (i & 1)));
        const u32 m = ((u32)i < full) ? ~0u : (((u32)i == full) ? ((1u << rem) - 1u) : 0u);
        r += (u32)__popc(h & m);
    }
    return r;
}
__device__ __forceinline__ void fm_mm_occ2(const u64 *__restrict__ vec, u64 lines, u32 v, u32 k1, u32 k2, u32 *r1, u32 *r2) {
    const u32 line1 = k1 / FM_LINE_BITS, line2 = k2 / FM_LINE_BITS;
    const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(vec + ((u64)v * lines + line1) * 8);
    ulonglong2 a = p[0], b = p[1], cc = p[2], d = p[3];
    *r1 = fm_mm_rank(a, b, cc, d, k1 - line1 * FM_LINE_BITS);
    if (line2 != line1) {
        const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(vec + ((u64)v * lines + line2) * 8);
        a = q[0]; b = q[1]; cc = q[2]; d = q[3];
    }
    *r2 = fm_mm_rank(a, b, cc, d, k2 - line2 * FM_LINE_BITS);
}

template <bool PAIRS, bool FILL>
__global__ __launch_bounds__(256, 8) void fm_mm_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ bits2, u64 lines,
                                                    const u32 *__restrict__ tab, const u32 *__restrict__ tab2, u32 sigma,
                                                    u32 N, u32 k, const u8 *__restrict__ pats,
                                                    const u64 *__restrict__ offs, u64 npat, i64 *__restrict__ out,
                                                    const u64 *__restrict__ hoffs, const u32 *__restrict__ sa,
                                                    u64 *__restrict__ hits, u8 *__restrict__ hit_mm) {
    __shared__ u32 s_tab[768];
    __shared__ u32 s_tab2[FM_PAIR_SIGMA * FM_PAIR_SIGMA];
    __shared__ uint4 s_frame[FM_MM_MAXK][256];
    for (int i = threadIdx.x; i < 768; i += 256) s_tab[i] = tab[i];
    if (PAIRS && threadIdx.x < FM_PAIR_SIGMA * FM_PAIR_SIGMA) s_tab2[threadIdx.x] = tab2[threadIdx.x];
    __syncthreads();
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= npat) return;
    const u64 m = offs[p + 1] - offs[p];
    const u8 *const pp = pats + offs[p];        // pp[j] = p[j]
    u32 cnt = 0;                // hits so far (< 2^32: every position is reported once)
    // the pattern is read right to left through an aligned window, as in fm_count_kernel (4 bytes here, one register: kept
    // as the window's number, counted from the aligned word that holds p[0]).  The aligned word that holds a valid byte
    // lies in that byte's page, so reading it whole is always safe.
    u32 widx = 0xFFFFFFFFu, word = 0;
    auto code_at = [&](u32 j) -> u32 {   // code of p[j], 0xFFFFFFFF for a byte the text does not hold
        const u32 t = ((u32)(uintptr_t)pp & 3u) + j;
        if ((t >> 2) != widx) {
            widx = t >> 2;
            word = *reinterpret_cast<const u32 *>(pp + j - (t & 3u));
        }
        return s_tab[(word >> (8 * (t & 3u))) & 255u];
    };
    // m = 0 answers 0 as tc_fm_count answers Nothing; m > n cannot occur in the text (and so q fits 32 bits)
    const bool live = m != 0 && m < (u64)N;
    if (k > FM_MM_MAXK) k = FM_MM_MAXK;         // (the entry points refuse a larger k: s_frame holds FM_MM_MAXK frames)
    u32 q = (u32)m, s = 1, e = N, alt = 0, d = 0;
    while (live) {
        if (q == 0) {                           // a variant that occurs: rows s - 1 .. e - 1, distance d
            if (FILL) {
                // (reports are rare beside steps: the segment's bounds are read again here instead of being kept)
                const u64 o = hoffs[p] + cnt, o_end = hoffs[p + 1];
                for (u32 r = s - 1, t = 0; r < e && o + t < o_end; r++, t++) {
                    hits[o + t] = sa ? (u64)sa[r] + 1 : (u64)r;
                    if (hit_mm) hit_mm[o + t] = (u8)d;
                }
            }
            cnt += e - s + 1;
        } else {
            const u32 own = code_at(q - 1);
            u32 c = own, nq = q - 1;
            const bool branch = d < k && alt < sigma;
            if (branch) {
                c = alt++;
                if (c == own) continue;
            }
            if (c != 0xFFFFFFFFu) {             // (no exact step from a byte the text does not hold: pop)
                u64 s2, e2;
                if (s == 1 && e == N) {         // the whole index (only ever the first step: C >= 1 afterwards)
                    s2 = (u64)s_tab[256 + c] + 1;
                    e2 = (u64)s_tab[256 + c] + s_tab[512 + c];
                } else {
                    const u64 *vec = bits;      // the vectors, the vector and the interval start of this step
                    u32 v = c, C = s_tab[256 + c];
                    if (PAIRS && !branch && d == k && q >= 2) {     // the exact tail, two symbols by one lookup
                        const u32 a = code_at(q - 2);
                        if (a != 0xFFFFFFFFu) {
                            vec = bits2;
                            v = a * sigma + c;
                            C = s_tab2[v];
                            nq = q - 2;
                        }
                    }
                    u32 o1, o2;
                    fm_mm_occ2(vec, lines, v, s - 1, e, &o1, &o2);
                    s2 = (u64)C + o1 + 1;
                    e2 = (u64)C + o2;
                }
                if (s2 <= e2 && e2 <= (u64)N) {
                    if (branch) s_frame[d++][threadIdx.x] = make_uint4(q, s, e, alt);
                    q = nq;
                    s = (u32)s2;
                    e = (u32)e2;
                    alt = 0;
                    continue;
                }
                if (branch) continue;           // this substitute does not occur: the next one
            }
        }
        if (d == 0) break;                      // pop
        const uint4 f = s_frame[--d][threadIdx.x];
        q = f.x; s = f.y; e = f.z; alt = f.w;
    }
    if (!FILL) out[p] = (i64)cnt;
}
