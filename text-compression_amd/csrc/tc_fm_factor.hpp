// tc_fm_factor.hpp -- FM-index factorize: the greedy longest-match parse of patterns against the indexed text, and the
// small kernels of its inverse (included by tc_fm_host.hpp, whose rank lines, tables, fm_mm_occ2 and walks it uses).  No
// counterpart in the reference.
//
// The parse of a pattern p of length m runs right to left, the direction backward search extends a match: with j = m,
// while j > 0, the phrase is the longest p[j - l .. j) that occurs in the text (inside it, never over its end).  l >= 1
// gives the match factor (pos, l), pos the 1-based text position of the occurrence in the FIRST row of the phrase's
// suffix-array interval, and j -= l; l = 0 means the byte p[j - 1] does not occur in the text at all and gives the literal
// factor (that byte's value, 0), j -= 1.  Extending to the left is exact -- if p[a .. j) occurs so does p[a + 1 .. j) --
// so the first empty interval ends the longest match.  Factors are stored in pattern order, left to right.
//
// The loop is the loop of fm_count_kernel that does not stop at the first empty interval: [s, e] (1-based, inclusive) is
// the interval of the phrase so far and len its length (0: no phrase is open).  A step is computed into (s2, e2) and only
// taken when it is not empty, so [s, e] is also "the interval before the last step": on an empty result the phrase closes
// at [s, e], row s - 1 is reported, and the next turn opens a phrase at the byte that failed: no line of the index is read
// twice (the byte itself is in the pattern window still, or one word away from it).  With pair vectors two symbols go per
// lookup; when a pair step comes back empty the first of its two symbols is retried as a single step from [s, e] -- the
// phrase may still grow by one byte -- and the phrase closes behind it: one extra line read per phrase end, none
// elsewhere.
//
// Termination.  Every turn of the loop consumes a pattern byte (q decreases) or closes a phrase (len > 0 becomes 0, and the
// turn behind it consumes a byte: a phrase is only opened by consuming one; a coded byte whose table interval is empty or
// leaves [1, N] is emitted as a literal), so the loop ends after at most 2 m turns on any index content.  What it reads.
// The index may be an imported byte string, i.e. caller data whose rank counts are arbitrary.  An interval is only ever
// stepped from when 1 <= s <= e <= N -- a step whose result is not of that shape counts as empty -- so the positions
// s - 1 < e <= N handed to fm_mm_occ2 lie in lines <= N / 448 < lines of the vector of a code < sigma (or of a pair
// < sigma^2); table entries are indexed by a byte, by such a code or by such a pair; the row looked up in the suffix array
// is s - 1 < N.  A phrase is closed at the latest when it is as long as the text.  On an index this library built no step
// is cut short.  An empty index has no tables (tab = null): every byte is a literal.
//
// FILL = false counts the factors of pattern p into cnt[p].  FILL = true repeats the identical parse and writes the
// pattern's own segment [foffs[p], foffs[p + 1]) from its back end forward -- the parse meets the factors right to left,
// so this is pattern order, with no atomics: fpos = sa[row] + 1 on a full index, the row itself on a sampled one (sa =
// null; fm_factor_walk_kernel then turns the rows of match factors into positions), flen = the phrase length; a literal is
// (byte, 0).
#pragma once

template <bool PAIRS, bool FILL>
__global__ __launch_bounds__(256, 8) void fm_factor_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ bits2,
                                                          u64 lines, const u32 *__restrict__ tab,
                                                          const u32 *__restrict__ tab2, u32 sigma, u32 N,
                                                          const u8 *__restrict__ pats, const u64 *__restrict__ offs,
                                                          u64 npat, i64 *__restrict__ cnt_out,
                                                          const u64 *__restrict__ foffs, const u32 *__restrict__ sa,
                                                          u64 *__restrict__ fpos, u32 *__restrict__ flen) {
    __shared__ u32 s_tab[768];
    __shared__ u32 s_tab2[FM_PAIR_SIGMA * FM_PAIR_SIGMA];
    for (int i = threadIdx.x; i < 768; i += 256) s_tab[i] = tab ? tab[i] : (i < 256 ? 0xFFFFFFFFu : 0u);
    if (PAIRS && threadIdx.x < FM_PAIR_SIGMA * FM_PAIR_SIGMA) s_tab2[threadIdx.x] = tab2[threadIdx.x];
    __syncthreads();
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= npat) return;
    const u8 *const pp = pats + offs[p];        // pp[j] = p[j]
    u64 q = offs[p + 1] - offs[p];              // bytes still to be consumed: the next one is pp[q - 1]
    u64 cnt = 0;                                // factors so far
    // the pattern is read right to left through an aligned 4-byte window, as in fm_mm_kernel (kept as the low bits of the
    // window's word address: consecutive reads lie at most two bytes apart, so equal numbers mean the same word).  The
    // aligned word that holds a valid byte lies in that byte's page, so reading it whole is always safe.
    u32 widx = 0, word = 0;
    auto load_window = [&](const u8 *ad) {
        widx = (u32)((uintptr_t)ad >> 2);
        word = *reinterpret_cast<const u32 *>((uintptr_t)ad & ~(uintptr_t)3);
    };
    auto byte_at = [&](u64 j) -> u32 {          // pp[j]
        const u8 *ad = pp + j;
        if ((u32)((uintptr_t)ad >> 2) != widx) load_window(ad);
        return (word >> (8 * ((u32)(uintptr_t)ad & 3u))) & 255u;
    };
    if (q) load_window(pp + q - 1);
    auto emit = [&](u64 pos_or_row, u32 len) {  // the next factor to the left
        if (FILL) {
            // (emits are rare beside steps: the segment's bounds are read again here instead of being kept)
            const u64 lo = foffs[p], hi = foffs[p + 1];
            if (cnt < hi - lo) {
                const u64 o = hi - 1 - cnt;
                fpos[o] = (len && sa) ? (u64)sa[pos_or_row] + 1 : pos_or_row;
                flen[o] = len;
            }
        }
        cnt++;
    };
    u32 s = 0, e = 0, len = 0;
    while (true) {
        if (q != 0) {
            const u32 byte = byte_at(q - 1);
            const u32 c = s_tab[byte];
            if (len == 0) {                     // open a phrase at this byte, or emit it as a literal
                u64 s2 = 1, e2 = 0;
                if (c != 0xFFFFFFFFu) {
                    s2 = (u64)s_tab[256 + c] + 1;
                    e2 = (u64)s_tab[256 + c] + s_tab[512 + c];
                }
                if (s2 <= e2 && e2 <= (u64)N) {
                    s = (u32)s2;
                    e = (u32)e2;
                    len = 1;
                } else {
                    emit(byte, 0);
                }
                q--;
                continue;
            }
            if (c != 0xFFFFFFFFu && len < N - 1) {
                bool last = false;              // a pair step came back empty: at most one more byte, then the phrase closes
                if (PAIRS && q >= 2) {          // two symbols by one lookup, when the one to the left occurs in the text too
                    const u32 a = s_tab[byte_at(q - 2)];
                    if (a != 0xFFFFFFFFu) {
                        const u32 pr = a * sigma + c;
                        u32 o1, o2;
                        fm_mm_occ2(bits2, lines, pr, s - 1, e, &o1, &o2);
                        const u64 s2 = (u64)s_tab2[pr] + o1 + 1, e2 = (u64)s_tab2[pr] + o2;
                        if (s2 <= e2 && e2 <= (u64)N) {
                            s = (u32)s2;
                            e = (u32)e2;
                            len += 2;
                            q -= 2;
                            continue;
                        }
                        last = true;
                    }
                }
                u32 o1, o2;
                fm_mm_occ2(bits, lines, c, s - 1, e, &o1, &o2);
                const u64 s2 = (u64)s_tab[256 + c] + o1 + 1, e2 = (u64)s_tab[256 + c] + o2;
                if (s2 <= e2 && e2 <= (u64)N) {
                    s = (u32)s2;
                    e = (u32)e2;
                    len++;
                    q--;
                    if (!last) continue;
                }
            }
        } else if (len == 0) {
            break;
        }
        emit(s - 1, len);                       // close the phrase at [s, e]: its first row
        len = 0;
    }
    if (!FILL) cnt_out[p] = (i64)cnt;
}

// ---- unfactorize: factor lists back to bytes, as one flat extract over all factors ---------------------------------------
// The factor offsets are caller data: they must not decrease (the entry has checked fac_offs[0] = 0 and read the factor
// total fac_offs[npat]; with both, every offset lies within the factor arrays).
__global__ __launch_bounds__(256) void fm_unfactor_offs_kernel(const u64 *__restrict__ fac_offs, u64 npat,
                                                               u32 *__restrict__ bad) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p < npat && fac_offs[p] > fac_offs[p + 1]) atomicOr(bad, 1u);
}

// One lane per factor, the plan of fm_extract_plan_kernel with literals: a match (len > 0) is the query (pos, len) of an
// extract -- 1 <= pos and pos - 1 + len <= n, tested without overflow -- with qlen = len bytes and qsegs = the rate-aligned
// segments it touches; a literal (len = 0) must be a byte value and is 1 byte and no segment.  A bad factor raises *bad and
// counts nothing.
__global__ __launch_bounds__(256) void fm_unfactor_plan_kernel(const u64 *__restrict__ fpos, const u32 *__restrict__ flen,
                                                               u64 nf, u64 n, u32 rate_log2, u64 *__restrict__ qlen,
                                                               u64 *__restrict__ qsegs, u32 *__restrict__ bad) {
    const u64 f = (u64)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const u64 pos = fpos[f], len = flen[f];
    u64 l = 0, sg = 0;
    if (len == 0) {
        if (pos > 255) atomicOr(bad, 1u); else l = 1;
    } else {
        const u64 a = pos - 1;          // (pos = 0 wraps to 2^64 - 1 > n)
        if (a > n || len > n - a) {
            atomicOr(bad, 1u);
        } else {
            l = len;
            sg = ((a + len - 1) >> rate_log2) - (a >> rate_log2) + 1;
        }
    }
    qlen[f] = l;
    qsegs[f] = sg;
}

// the literals' bytes (the matches' bytes are fm_extract_walk_kernel's, which writes nothing outside a match's own range)
__global__ __launch_bounds__(256) void fm_unfactor_literal_kernel(const u64 *__restrict__ fpos, const u32 *__restrict__ flen,
                                                                  u64 nf, const u64 *__restrict__ boffs,
                                                                  u8 *__restrict__ out) {
    const u64 f = (u64)blockIdx.x * 256 + threadIdx.x;
    if (f < nf && flen[f] == 0) out[boffs[f]] = (u8)fpos[f];
}

// out_offs[p] = the byte offset of pattern p's first factor, p = 0 .. npat (boffs[nf] = the byte total)
__global__ __launch_bounds__(256) void fm_unfactor_gather_kernel(const u64 *__restrict__ fac_offs, u64 npat,
                                                                 const u64 *__restrict__ boffs, u64 *__restrict__ out_offs) {
    const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p <= npat) out_offs[p] = boffs[fac_offs[p]];
}
