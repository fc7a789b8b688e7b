// tc_fm_host.hpp -- FM-index: build, batched count, locate, extract, factorize, matching statistics.
//
// Replaces (reference FMIndex/Internal.hs) seqToCc :275-316 (C[c], there derived
// from an O(n^2) rotation matrix, BWT/Internal.hs:209-241; here a byte histogram),
// seqToOccCK :195-259 (a full sigma x N table of inclusive counts; here one rank
// bit-vector per present byte: 64-byte lines = {u64 ones-before, 7 x u64 bits}, so
// every Occ(c,k) lookup touches exactly one line), countFMIndex :347-438 and
// locateFMIndex :448-542 mapped over the pattern list (FMIndex.hs:362-379,
// 411-432, 475-497: serial or parListChunk sparks; here one lane per pattern in one
// launch, result order = pattern order).
//
// Two symbols per step (round 3).  One backward-search step is one dependent random 64-byte line read, and the
// batch of BASELINE configs[3] runs at the rate the memory system serves such reads (50 G lines/s from 2^27-byte
// texts on, whatever the index size: scripts/fm_sweep.py) -- so the lever is the NUMBER of dependent reads.  For
// texts of at most FM_PAIR_SIGMA byte values a second set of rank bit-vectors is kept, one per PAIR (a, b) of
// byte values: bit j is set iff row j's suffix is preceded by "ab" (L[j] = b and T[SA[j] - 2] = a).  With
// C2[ab] = C[a] + Occ(a, C[b]) (the start of the "ab" interval) two pattern symbols are consumed by one lookup:
//   s' = C2[ab] + Occ2(ab, s - 1) + 1,  e' = C2[ab] + Occ2(ab, e)
// which is exactly what two steps of countFMIndex (:424-432) compute, because the rows with pair ab inside a
// range keep their relative order among the "ab"-prefixed suffixes.  The reference's stop rules stay as they
// are: the range is tested for emptiness before every (single or double) step (:387-389), a byte that is not
// in the text stops the loop where the reference stops it (:393,:421) -- a pair is only taken when both of its
// bytes occur -- and an empty range between the two symbols of a pair stays empty, so the result (0 = Nothing)
// is the same.  Cost: sigma^2 / 7 bytes per text byte (3.6 N for ACGTN).
#pragma once
#include "tc_decode_host.hpp"
#include "tc_lcp_host.hpp"   // lcp_device: the LCP part of an index (tc_fm_build_lcp)

#define FM_LINE_BITS 448  // 7 words of payload per 64-byte line
#define FM_PAIR_SIGMA 5   // pair vectors for texts of at most this many byte values (25 vectors)
#define FM_LCP_FANOUT 64  // fan-out of the min tree over the LCP array (tc_dbg_fm_set_lcp_fanout builds 4, 8 or 16 for the tests)

struct tc_fm {
    int device = 0;
    u64 n = 0, N = 0, primary = 0;
    u32 sigma_bytes = 0;  // present byte values
    u8 *d_L = nullptr;
    u32 *d_sa = nullptr;
    u64 *d_bits = nullptr;  // [sigma_bytes][lines][8]
    u32 *d_tab = nullptr;   // [0..255] code of byte (0xFFFFFFFF absent), [256..511] C[code], [512..767] cnt[code]
    u64 *d_bits2 = nullptr; // [sigma_bytes^2][lines][8]: one rank bit-vector per pair of byte values (or null)
    u32 *d_tab2 = nullptr;  // [FM_PAIR_SIGMA^2] C2[a * sigma_bytes + b]
    void *bits2_chunks = nullptr;   // d_bits2 as mapped chunks (tc_chunked_alloc) instead of one hipMalloc block, or null
    u64 lines = 0;
    u32 counts[256];
    i16 sym_of_code[256];
    // the locate part.  sa_rate 1: d_L + d_sa (the full suffix array).  sa_rate k > 1 (tc_fm_build_sampled): d_L + d_marks +
    // d_samples and no d_sa -- marks is one more rank bit-vector in the line format above, bit j set iff SA[j] % k == 0 (the
    // primary row, SA = 0, is always marked and, unlike in the symbol vectors, takes part); samples holds the marked rows'
    // SA values in ROW order: samples[rank_marks(j)] = SA[j], floor(n / k) + 1 of them.  sa_rate 0: no locate part.
    u32 sa_rate = 0;
    u64 *d_marks = nullptr;   // [lines][8]
    u32 *d_samples = nullptr; // [nsamples]
    u64 nsamples = 0;
    // the extract part (tc_fm_build_self; independent of sa_rate): text_rate k >= 1 keeps the ROW of every k-th text position,
    // d_isa[i] = the row j with SA[j] = i * k, i = 0 .. floor(n / k) -- 4 / k bytes per text byte.  text_rate 0: none.
    u32 text_rate = 0;
    u32 *d_isa = nullptr;     // [nisa]
    u64 nisa = 0;             // n / text_rate + 1
    // the LCP part (tc_fm_build_lcp; never exported or imported): d_lcp = the array tc_lcp_array_dev defines over the N rows,
    // d_lmin = the min tree over it (tc_fm_ms.hpp: fm_ms_tree_shape gives the levels), fan-out 2^lcp_fan_log2
    u32 *d_lcp = nullptr;     // [N]
    u32 *d_lmin = nullptr;    // [lmin_words]
    u64 lmin_words = 0;
    u32 lcp_fan_log2 = 0;
};

#ifdef __HIPCC__

// one wave per line: ballots of (symbol == c) for the line's 7 words
__global__ __launch_bounds__(256) void fm_bits_kernel(const u8 *__restrict__ L, u64 N, u64 primary,
                                                      const u32 *__restrict__ tab, u32 sigma,
                                                      u64 lines, u64 *__restrict__ bits) {
    __shared__ u32 s_code[256];
    s_code[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    const u64 line = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= lines) return;
    const u32 l = threadIdx.x & 63;
    u32 sw[7];
#pragma unroll
    for (int w = 0; w < 7; w++) {
        u64 j = line * FM_LINE_BITS + (u64)w * 64 + l;
        sw[w] = (j < N && j != primary) ? s_code[L[j]] : 0xFFFFFFFFu;
    }
    for (u32 c = 0; c < sigma; c++) {
        u64 mine = 0;
        u32 pc = 0;
#pragma unroll
        for (int w = 0; w < 7; w++) {
            u64 m = __ballot(sw[w] == c);
            pc += (u32)__popcll(m);
            if ((int)l == w + 1) mine = m;
        }
        if (l == 0) mine = pc;  // ones in this line; made cumulative by fm_scan_kernel
        if (l < 8) bits[((u64)c * lines + line) * 8 + l] = mine;
    }
}

// per symbol: exclusive scan of the line counts (word 0 of each line); block c
__global__ __launch_bounds__(1024) void fm_scan_kernel(u64 *bits, u64 lines) {
    __shared__ u64 s_part[1024];
    u64 *b = bits + (u64)blockIdx.x * lines * 8;
    u64 per = (lines + 1023) / 1024;
    u64 lo = threadIdx.x * per, hi = lo + per < lines ? lo + per : lines;
    u64 v = 0;
    for (u64 t = lo; t < hi; t++) v += b[t * 8];
    s_part[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = 0;
        for (int i = 0; i < 1024; i++) {
            u64 c = s_part[i];
            s_part[i] = run;
            run += c;
        }
    }
    __syncthreads();
    u64 run = s_part[threadIdx.x];
    for (u64 t = lo; t < hi; t++) {
        u64 c = b[t * 8];
        b[t * 8] = run;
        run += c;
    }
}

// the pair vectors: row j carries pair (a, b) = (T[SA[j] - 2], L[j]) when SA[j] >= 2 (a row whose suffix starts at
// text position 0 or 1 has no pair: nothing can be matched two symbols to its left)
__global__ __launch_bounds__(256) void fm_bits2_kernel(const u8 *__restrict__ L, const u32 *__restrict__ sa,
                                                       const u8 *__restrict__ text, u64 N,
                                                       const u32 *__restrict__ tab, u32 sigma, u64 lines,
                                                       u64 *__restrict__ bits2) {
    __shared__ u32 s_code[256];
    s_code[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    const u64 line = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= lines) return;
    const u32 l = threadIdx.x & 63;
    u32 sw[7];
#pragma unroll
    for (int w = 0; w < 7; w++) {
        const u64 j = line * FM_LINE_BITS + (u64)w * 64 + l;
        u32 pc = 0xFFFFFFFFu;
        if (j < N) {
            const u32 p = sa[j];
            if (p >= 2) pc = s_code[text[p - 2]] * sigma + s_code[L[j]];
        }
        sw[w] = pc;
    }
    for (u32 c = 0; c < sigma * sigma; c++) {
        u64 mine = 0;
        u32 pc = 0;
#pragma unroll
        for (int w = 0; w < 7; w++) {
            const u64 m = __ballot(sw[w] == c);
            pc += (u32)__popcll(m);
            if ((int)l == w + 1) mine = m;
        }
        if (l == 0) mine = pc;
        if (l < 8) bits2[((u64)c * lines + line) * 8 + l] = mine;
    }
}

#include "tc_fm_count.hpp"   // fm_occ, fm_occ2: the rank lookups; fm_count_lane: the backward search of one pattern

// C2[a * sigma + b] = C[a] + Occ(a, C[b]): the 0-based start of the interval of suffixes that begin with "ab"
__global__ void fm_c2_kernel(const u64 *__restrict__ bits, u64 lines, const u32 *__restrict__ tab, u32 sigma,
                             u32 *__restrict__ tab2) {
    const u32 t = threadIdx.x;
    if (t >= sigma * sigma) return;
    const u32 a = t / sigma, b = t % sigma;
    tab2[t] = tab[256 + a] + (u32)fm_occ(bits, lines, a, (u64)tab[256 + b]);
}

// countFMIndex (FMIndex/Internal.hs:347-438), one pattern per lane (the loop: fm_count_lane, tc_fm_count.hpp).
// ranges (optional): [2p] = s, [2p+1] = e (1-based inclusive) for non-empty results, 0 0 otherwise.
// The index may be an imported byte string, i.e. caller data.  The rule for every query on such an index: a malformed body
// is answered by TC_ERR_MALFORMED, at import or at the query, or by TC_OK with the answer the contents define, and every
// kernel stays inside the index's parts.  Here: an interval is only stepped from, counted or written as a range when
// 1 <= s <= e <= N (N = the rows of the index), so no rank count, however wrong, moves a read outside the vectors, and
// the ranges that fm_locate_fill_kernel, fm_locate_rows_kernel and fm_offsets_of_counts take from this kernel hold rows
// below N and at most N of them per pattern.  tests/fm_wire_ref.py states the answers, tests/test_gpu_fm_import_foreign.py
// and host/check/fm_count_kernels.cpp (the same loop under a host sanitizer) hold the kernel to them.
template <bool PAIRS>
__global__ __launch_bounds__(256) void fm_count_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ bits2,
                                                       u64 lines, const u32 *__restrict__ tab,
                                                       const u32 *__restrict__ tab2, u32 sigma, u64 N,
                                                       const u8 *__restrict__ pats,
                                                       const u64 *__restrict__ offs, u64 npat,
                                                       i64 *__restrict__ out,
                                                       u64 *__restrict__ ranges) {
    __shared__ u32 s_tab[768];
    __shared__ u32 s_tab2[FM_PAIR_SIGMA * FM_PAIR_SIGMA];
    for (int i = threadIdx.x; i < 768; i += 256) s_tab[i] = tab[i];
    if (PAIRS && threadIdx.x < FM_PAIR_SIGMA * FM_PAIR_SIGMA) s_tab2[threadIdx.x] = tab2[threadIdx.x];
    __syncthreads();
    u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p >= npat) return;
    u64 s = 0, e = 0;
    const i64 cnt = fm_count_lane<PAIRS>(bits, bits2, lines, s_tab, s_tab2, sigma, N, pats, offs[p], offs[p + 1], &s, &e);
    out[p] = cnt;
    if (ranges) {
        ranges[2 * p] = s;
        ranges[2 * p + 1] = e;
    }
}

__global__ __launch_bounds__(256) void fm_cnt_to_u64_kernel(const i64 *__restrict__ cnt, u64 npat,
                                                            u64 *__restrict__ len) {
    u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    if (p < npat) len[p] = (u64)cnt[p];
}

// locate: hits[off[p] + t] = sa[s - 1 + t] + 1 (FMIndex.hs:496: suffixstartpos, 1-based)
__global__ __launch_bounds__(256) void fm_locate_fill_kernel(const u64 *__restrict__ ranges,
                                                             const u64 *__restrict__ hoffs,
                                                             const u32 *__restrict__ sa, u64 npat,
                                                             u64 cap, u64 *__restrict__ hits) {
    u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    bool in = p < npat;
    u64 s = in ? ranges[2 * p] : 0, e = in ? ranges[2 * p + 1] : 0;
    u64 o = in ? hoffs[p] : 0;
    u64 len = (in && s) ? e - s + 1 : 0;
    const u64 LONG = 32;
    if (len && len < LONG)
        for (u64 t = 0; t < len; t++)
            if (o + t < cap) hits[o + t] = (u64)sa[s - 1 + t] + 1;
    u64 longmask = __ballot(len >= LONG);
    while (longmask) {
        int src = __builtin_ctzll(longmask);
        longmask &= longmask - 1;
        u64 ls = __shfl(s, src, 64), ll = __shfl(len, src, 64), lo = __shfl(o, src, 64);
        for (u64 t = lane_id(); t < ll; t += 64)
            if (lo + t < cap) hits[lo + t] = (u64)sa[ls - 1 + t] + 1;
    }
}

// ---- locate from a sampled suffix array --------------------------------------------------------------------------
// the marks vector of a sampled index: one wave per line, ballots of (SA[j] % rate == 0); word 0 = the line's ones,
// made cumulative by fm_scan_kernel like every other vector
__global__ __launch_bounds__(256) void fm_marks_kernel(const u32 *__restrict__ sa, u64 N, u32 rate, u64 lines,
                                                       u64 *__restrict__ marks) {
    const u64 line = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= lines) return;
    const u32 l = threadIdx.x & 63;
    u64 mine = 0;
    u32 pc = 0;
#pragma unroll
    for (int w = 0; w < 7; w++) {
        const u64 j = line * FM_LINE_BITS + (u64)w * 64 + l;
        const u64 m = __ballot(j < N && (sa[j] & (rate - 1)) == 0);
        pc += (u32)__popcll(m);
        if ((int)l == w + 1) mine = m;
    }
    if (l == 0) mine = pc;
    if (l < 8) marks[line * 8 + l] = mine;
}

// ordered compaction of the sampled entries (after the scan): samples[rank_marks(j)] = SA[j] for every marked row j
__global__ __launch_bounds__(256) void fm_samples_kernel(const u32 *__restrict__ sa, u64 N, u64 lines,
                                                         const u64 *__restrict__ marks, u64 nsamples,
                                                         u32 *__restrict__ samples) {
    const u64 line = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= lines) return;
    const u32 l = threadIdx.x & 63;
    u64 base = marks[line * 8];
#pragma unroll
    for (int w = 0; w < 7; w++) {
        const u64 m = marks[line * 8 + 1 + w];
        const u64 j = line * FM_LINE_BITS + (u64)w * 64 + l;
        if (((m >> l) & 1) && j < N) {
            const u64 idx = base + (u64)__popcll(m & lanemask_lt());
            if (idx < nsamples) samples[idx] = sa[j];
        }
        base += (u64)__popcll(m);
    }
}

// ones of a whole vector (import check: the marks of a sampled index must hold exactly nsamples ones); *total zeroed before
__global__ __launch_bounds__(256) void fm_popcount_kernel(const u64 *__restrict__ bits, u64 lines,
                                                          unsigned long long *__restrict__ total) {
    u32 pc = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < lines * 8; i += (u64)gridDim.x * 256)
        if (i & 7) pc += (u32)__popcll(bits[i]);
    pc = wave_sum(pc);
    if (lane_id() == 0 && pc) atomicAdd(total, (unsigned long long)pc);
}

// fm_locate_fill_kernel for a sampled index: hits[off[p] + t] = the ROW s - 1 + t (0-based) of the hit; fm_locate_walk_kernel
// turns rows into positions
__global__ __launch_bounds__(256) void fm_locate_rows_kernel(const u64 *__restrict__ ranges,
                                                             const u64 *__restrict__ hoffs, u64 npat,
                                                             u64 cap, u64 *__restrict__ hits) {
    u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
    bool in = p < npat;
    u64 s = in ? ranges[2 * p] : 0, e = in ? ranges[2 * p + 1] : 0;
    u64 o = in ? hoffs[p] : 0;
    u64 len = (in && s) ? e - s + 1 : 0;
    const u64 LONG = 32;
    if (len && len < LONG)
        for (u64 t = 0; t < len; t++)
            if (o + t < cap) hits[o + t] = s - 1 + t;
    u64 longmask = __ballot(len >= LONG);
    while (longmask) {
        int src = __builtin_ctzll(longmask);
        longmask &= longmask - 1;
        u64 ls = __shfl(s, src, 64), ll = __shfl(len, src, 64), lo = __shfl(o, src, 64);
        for (u64 t = lane_id(); t < ll; t += 64)
            if (lo + t < cap) hits[lo + t] = ls - 1 + t;
    }
}

#define FM_ERR_WALK 0x4000u   // device error bit of a walk that ran into one of its bounds (in 0xff00: TC_ERR_MALFORMED)

// One lane per HIT, flat over all hits of the batch: row -> text position by walking the LF mapping to the next sampled row.
//   steps = 0; while row is not marked: c = code(L[row]); row = C[c] + Occ(c, row); steps++
//   hits[h] = samples[rank_marks(row)] + steps + 1
// with the index's own conventions: rows are 0-based, tab[256 + c] = C[c] counts the '$' row (it starts at 1), Occ(c, k)
// counts L[0 .. k) without the primary row -- LF(j) = C + Occ(c, j) is the 0-based form of the s' = C + Occ(c, s - 1) + 1
// of fm_count_kernel -- and SA[LF(j)] = SA[j] - 1, so a row `steps` steps before a sample of value v has SA = v + steps;
// the answer is 1-based (FMIndex.hs:496).  SA = 0 (the primary row, whose L is Nothing) is a multiple of every rate: a walk
// on a well-formed index ends there at the latest and never steps from it.
// A step is two dependent levels of random reads: {the L byte, the marks line} of the row, issued together, then the rank
// line of (c, row).  Lanes leave the loop after different step counts (0 .. rate - 1); nothing in it is cross-lane.
// The index may be an imported byte string, i.e. caller data: every row is kept < N, every sample index < nsamples, the
// loop ends after rate - 1 steps, a byte without a code or a step from the primary row stops the walk, and a position must
// be a multiple of the rate plus the steps and lie in the text; a lane that runs into any of these raises FM_ERR_WALK (the
// call answers TC_ERR_MALFORMED) and writes 0.  So no content can make the kernel spin or read outside L [N + 16], the
// vectors [lines = N / 448 + 1 lines each] and samples [nsamples].
// (the body of two kernels: skip = null for locate; for factorize skip[h] = 0 marks an entry that is no row -- a literal
// factor -- and is left as it is)
__device__ __forceinline__ void fm_locate_walk_body(const u64 *__restrict__ bits, const u64 *__restrict__ marks,
                                                    u64 lines, const u32 *__restrict__ tab, u32 sigma,
                                                    const u8 *__restrict__ L, const u32 *__restrict__ samples,
                                                    u64 nsamples, u64 N, u64 primary, u32 rate, u64 total,
                                                    u64 *__restrict__ hits, u32 *__restrict__ err,
                                                    const u32 *__restrict__ skip) {
    __shared__ u32 s_tab[512];
    for (int i = threadIdx.x; i < 512; i += 256) s_tab[i] = tab[i];
    __syncthreads();
    const u64 h = (u64)blockIdx.x * 256 + threadIdx.x;
    if (h >= total) return;
    if (skip && skip[h] == 0) return;
    u64 row = hits[h];
    bool bad = row >= N;
    if (bad) row = 0;
    u32 steps = 0;
    u64 pos = 0;
    while (true) {
        const u32 byte = L[row];
        const u64 line = row / FM_LINE_BITS;
        const u32 off = (u32)(row - line * FM_LINE_BITS);
        const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(marks + line * 8);
        const ulonglong2 a = p[0], b = p[1], cc = p[2], d = p[3];
        const u64 w[7] = {a.y, b.x, b.y, cc.x, cc.y, d.x, d.y};
        u64 r = a.x, cur = 0;
        const u32 full = off >> 6, rem = off & 63;
#pragma unroll
        for (int i = 0; i < 7; i++) {
            const u64 m = ((u32)i < full) ? ~0ull : (((u32)i == full) ? ((1ull << rem) - 1ull) : 0ull);
            r += (u64)__popcll(w[i] & m);
            if ((u32)i == full) cur = w[i];
        }
        if ((cur >> rem) & 1) {            // a sampled row: r = rank_marks(row)
            if (r >= nsamples) { bad = true; break; }
            const u64 v = samples[r];
            pos = v + steps;
            if ((v & (rate - 1)) != 0 || pos >= N) bad = true;
            break;
        }
        const u32 c = s_tab[byte];
        if (steps + 1 >= rate || row == primary || c >= sigma) { bad = true; break; }
        const u64 nr = (u64)s_tab[256 + c] + fm_occ(bits, lines, c, row);
        if (nr >= N) { bad = true; break; }
        row = nr;
        steps++;
    }
    if (bad) atomicOr(err, FM_ERR_WALK);
    hits[h] = bad ? 0 : pos + 1;
}
__global__ __launch_bounds__(256) void fm_locate_walk_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ marks,
                                                             u64 lines, const u32 *__restrict__ tab, u32 sigma,
                                                             const u8 *__restrict__ L, const u32 *__restrict__ samples,
                                                             u64 nsamples, u64 N, u64 primary, u32 rate, u64 total,
                                                             u64 *__restrict__ hits, u32 *__restrict__ err) {
    fm_locate_walk_body(bits, marks, lines, tab, sigma, L, samples, nsamples, N, primary, rate, total, hits, err, nullptr);
}
// the walk over a factor list (tc_fm_factor.hpp): fpos[f] of a match factor (flen[f] > 0) is a row; literals are skipped
__global__ __launch_bounds__(256) void fm_factor_walk_kernel(const u64 *__restrict__ bits, const u64 *__restrict__ marks,
                                                             u64 lines, const u32 *__restrict__ tab, u32 sigma,
                                                             const u8 *__restrict__ L, const u32 *__restrict__ samples,
                                                             u64 nsamples, u64 N, u64 primary, u32 rate, u64 total,
                                                             u64 *__restrict__ fpos, const u32 *__restrict__ flen,
                                                             u32 *__restrict__ err) {
    fm_locate_walk_body(bits, marks, lines, tab, sigma, L, samples, nsamples, N, primary, rate, total, fpos, err, flen);
}

// ---- extract: text ranges read back from the index -----------------------------------------------------------------
// The text samples (the opposite direction of the locate samples): isa[k] = the row j with SA[j] = k * rate, for
// k = 0 .. floor(n / rate).  One pass over the suffix array -- the index's own for a full index, the copy in the workspace
// for a sampled one, where fm_marks_kernel reads it -- scatters the rows whose suffix starts at a multiple of the rate.
// Every multiple of the rate up to n is the start of exactly one suffix, so every entry is written exactly once.  The
// empty suffix (position n) is row 0 in every suffix array sa_build makes -- Nothing sorts first: tab[256 + c] = C[c]
// starts at 1 for that row (fm_make_tab) -- so the walk that starts at the end of the text needs no sample; when n is a
// multiple of the rate the scatter stores that 0 at isa[n / rate] like any other entry.
__global__ __launch_bounds__(256) void fm_isa_kernel(const u32 *__restrict__ sa, u64 N, u32 rate, u32 rate_log2, u64 nisa,
                                                     u32 *__restrict__ isa) {
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < N; j += (u64)gridDim.x * 256) {
        const u32 v = sa[j];
        const u64 k = v >> rate_log2;
        if ((v & (rate - 1)) == 0 && k < nisa) isa[k] = (u32)j;
    }
}

// import check of the text samples: res[0] = the largest sample (every one must be < N), res[1] = isa[0] (must be the
// primary row, the row of SA = 0); res zeroed before
__global__ __launch_bounds__(256) void fm_isa_max_kernel(const u32 *__restrict__ isa, u64 nisa, u32 *__restrict__ res) {
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < nisa; i += (u64)gridDim.x * 256) m = isa[i] > m ? isa[i] : m;
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
    }
    if (lane_id() == 0 && m) atomicMax(res, m);
    if (blockIdx.x == 0 && threadIdx.x == 0) res[1] = isa[0];
}

// One lane per query (start, len), start 1-based as locate answers positions: a = start - 1, e = a + len must satisfy
// start >= 1 and e <= n (tested without overflow).  qlen[q] = len and qsegs[q] = the number of rate-aligned segments
// [k * rate, (k + 1) * rate) that [a, e) touches, both 0 for a bad query, which also raises *bad; two exclusive scans of
// them give the output offsets and the segment offsets.
__global__ __launch_bounds__(256) void fm_extract_plan_kernel(const u64 *__restrict__ starts, const u64 *__restrict__ lens,
                                                              u64 nq, u64 n, u32 rate_log2, u64 *__restrict__ qlen,
                                                              u64 *__restrict__ qsegs, u32 *__restrict__ bad) {
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const u64 a = starts[q] - 1, len = lens[q];
    u64 l = 0, sg = 0;
    if (a > n || len > n - a) {     // (start = 0 wraps to 2^64 - 1 > n)
        atomicOr(bad, 1u);
    } else if (len) {
        l = len;
        sg = ((a + len - 1) >> rate_log2) - (a >> rate_log2) + 1;
    }
    qlen[q] = l;
    qsegs[q] = sg;
}

// One lane per (query, segment): segment k of a query [a, e) is the text [max(a, k * rate), min(e, (k + 1) * rate)), read
// by an LF walk from the anchor q = min((k + 1) * rate, n), whose row is isa[k + 1] (row 0 for q = n):
//   for p = q - 1 down to max(a, k * rate): byte = L[row]; if p < e: out[out_offs[query] + p - a] = byte; row = LF(row)
// with LF(row) = C[code(byte)] + Occ(code, row), the step of fm_locate_walk_kernel: L[row] = T[SA[row] - 1] and
// SA[LF(row)] = SA[row] - 1.  The step count is fixed by the arguments (<= rate), the last byte of a segment needs no step
// behind it, and only a query's last segment reads bytes it does not emit (q - e < rate of them).  A step is two dependent
// random reads: the L byte, then the rank line of (code, row) -- one fewer than a locate step, which also reads the marks
// line.
// item -> query: the largest query index whose segment offset is <= the item (a search in the scanned offsets; queries
// without segments share their successor's offset and are skipped by it).
// Bytes arrive in descending address order: they are gathered in a 64-bit register and stored as one word when the walk
// crosses an aligned 8-byte boundary of the output, the two ragged ends of the lane's range by byte stores.  Neighbouring
// segments of a query belong to other lanes: nothing is written outside the lane's own range.
// The index may be imported, i.e. caller data: every row is kept < N and the sample index < nisa, a byte without a code
// stops the walk and so does a step FROM the primary row (its L byte is a placeholder 0; a correct walk reaches that row
// only behind its last step, at p = 0, and never reads its byte).  A lane that runs into one of these raises FM_ERR_WALK (the
// call answers TC_ERR_MALFORMED) and fills its range with zeros.
__device__ __forceinline__ void fm_extract_flush(u8 *base, u64 acc, u32 cnt) {   // base[j] = byte j of acc, j < cnt
    for (u32 j = 0; j < cnt; j++) base[j] = (u8)(acc >> (8 * j));
}
__global__ __launch_bounds__(256) void fm_extract_walk_kernel(const u64 *__restrict__ bits, u64 lines,
                                                              const u32 *__restrict__ tab, u32 sigma,
                                                              const u8 *__restrict__ L, const u32 *__restrict__ isa,
                                                              u64 nisa, u64 N, u64 primary, u32 rate_log2,
                                                              const u64 *__restrict__ starts, const u64 *__restrict__ lens,
                                                              const u64 *__restrict__ seg_offs,
                                                              const u64 *__restrict__ out_offs, u64 nq, u64 nsegs,
                                                              u8 *__restrict__ out, u32 *__restrict__ err) {
    __shared__ u32 s_tab[512];
    for (int i = threadIdx.x; i < 512; i += 256) s_tab[i] = tab[i];
    __syncthreads();
    const u64 item = (u64)blockIdx.x * 256 + threadIdx.x;
    if (item >= nsegs) return;
    u64 lo_q = 0, hi_q = nq;            // seg_offs[lo_q] <= item < seg_offs[hi_q] (seg_offs[0] = 0, seg_offs[nq] = nsegs)
    while (hi_q - lo_q > 1) {
        const u64 mid = lo_q + ((hi_q - lo_q) >> 1);
        if (seg_offs[mid] <= item) lo_q = mid; else hi_q = mid;
    }
    const u64 n = N - 1;
    const u64 a = starts[lo_q] - 1, e = a + lens[lo_q];
    const u64 k = (a >> rate_log2) + (item - seg_offs[lo_q]);
    const u64 seg_lo = k << rate_log2, seg_hi = (k + 1) << rate_log2;
    const u64 lo = a > seg_lo ? a : seg_lo;
    const u64 anchor = seg_hi < n ? seg_hi : n;
    const u64 top = e < anchor ? e : anchor;        // this lane emits [lo, top)
    u8 *const o = out + out_offs[lo_q] - a;         // o + p: where text position p goes
    bool bad = false;
    u64 row = 0;
    if (anchor != n) {
        if (k + 1 < nisa) row = isa[k + 1]; else bad = true;
        if (row >= N) { bad = true; row = 0; }
    }
    u64 acc = 0;
    u32 cnt = 0;
    if (!bad && lo < anchor) {
        for (u64 p = anchor - 1;; p--) {
            if (row == primary) { bad = true; break; }
            const u32 byte = L[row];
            const u32 c = s_tab[byte];
            if (c >= sigma) { bad = true; break; }
            if (p < top) {
                u8 *const ad = o + p;
                acc = (acc << 8) | byte;
                cnt++;
                if (((uintptr_t)ad & 7) == 0) {
                    if (cnt == 8) *reinterpret_cast<u64 *>(ad) = acc;
                    else fm_extract_flush(ad, acc, cnt);
                    cnt = 0;
                }
            }
            if (p == lo) break;
            const u64 nr = (u64)s_tab[256 + c] + fm_occ(bits, lines, c, row);
            if (nr >= N) { bad = true; break; }
            row = nr;
        }
    }
    if (bad) {
        atomicOr(err, FM_ERR_WALK);
        for (u64 p = lo; p < top; p++) o[p] = 0;
    } else if (cnt) {
        fm_extract_flush(o + lo, acc, cnt);
    }
}

#include "tc_fm_mm.hpp"   // fm_mm_kernel: count / locate within Hamming distance k
#include "tc_fm_factor.hpp"   // fm_factor_kernel: the longest-match parse; the small kernels of its inverse
#include "tc_fm_ms.hpp"   // fm_ms_kernel: matching statistics; the min tree over the LCP array; the small kernels of the MEMs
static inline u32 fm_log2(u32 v) { return 31u - (u32)__builtin_clz(v); }   // v: a power of two
#include "tc_esa_plan.hpp"   // MinTree: the shape and the build of that tree

#endif  // __HIPCC__

// code of byte / C[code] / count[code] from the byte histogram; returns the number of present byte values
static u32 fm_make_tab(const u32 *counts, u32 *tab, i16 *sym_of_code) {
    u32 sig = 0, acc = 1;
    for (int b = 0; b < 256; b++) {
        tab[b] = 0xFFFFFFFFu;
        if (counts[b]) {
            tab[b] = sig;
            tab[256 + sig] = acc;
            tab[512 + sig] = counts[b];
            if (sym_of_code) sym_of_code[sig] = (i16)b;
            acc += counts[b];
            sig++;
        }
    }
    for (u32 c = sig; c < 256; c++) tab[256 + c] = tab[512 + c] = 0;
    return sig;
}

static void fm_release(tc_fm *fm) {
    if (!fm) return;
    (void)hipSetDevice(fm->device);
    if (fm->d_L) (void)hipFree(fm->d_L);
    if (fm->d_sa) (void)hipFree(fm->d_sa);
    if (fm->d_marks) (void)hipFree(fm->d_marks);
    if (fm->d_samples) (void)hipFree(fm->d_samples);
    if (fm->d_isa) (void)hipFree(fm->d_isa);
    if (fm->d_lcp) (void)hipFree(fm->d_lcp);
    if (fm->d_lmin) (void)hipFree(fm->d_lmin);
    if (fm->d_bits) (void)hipFree(fm->d_bits);
    if (fm->bits2_chunks) tc_chunked_free(fm->bits2_chunks);
    else if (fm->d_bits2) (void)hipFree(fm->d_bits2);
    if (fm->d_tab2) (void)hipFree(fm->d_tab2);
    if (fm->d_tab) (void)hipFree(fm->d_tab);
    delete fm;
}

// the pair vectors of a long text are gigabytes (3.6 bytes per text byte): with TC_FM_VMM = 21 .. 34 and from TC_FM_VMM_MIN_LOG2 (default 2^31 bytes) on
// they are mapped from 2^TC_FM_VMM-byte chunks like the workspace of a long record (default 0: one hipMalloc block -- the experiment
// of round 4: the count rate at 2^30 bytes of text does not depend on how the vectors are mapped)
static void fm_alloc_bits2(tc_ctx *ctx, tc_fm *fm, size_t bytes) {
    const int lg = env_int("TC_FM_VMM", 0);   // (measured, round 4: no gain -- profiles/r04_fm_sweep.txt -- so off unless asked for)
    if (lg >= 21 && lg <= 34 && bytes >= ((size_t)1 << env_int("TC_FM_VMM_MIN_LOG2", 31))) {
        void *p = tc_chunked_alloc(ctx, bytes, lg, &fm->bits2_chunks);
        if (p) {
            fm->d_bits2 = static_cast<u64 *>(p);
            return;
        }
    }
    TC_HIP(ctx, hipMalloc((void **)&fm->d_bits2, bytes));
}

// text_host or text_dev (a text already in HBM is used where it lies: no copy at all)
// sa_rate 1: the index owns the full suffix array.  sa_rate k > 1: the suffix array lives in the context's workspace for the
// duration of the call (the same peak: the 4 N bytes are carved there instead of allocated) and the index keeps marks + samples.
// text_rate k >= 1: the index also keeps the text samples (d_isa), scattered from the same suffix array before it goes.
// with_lcp: the index also keeps the LCP array and its min tree, made by lcp_device while the text and the full suffix array
// are still there (both in the workspace on a sampled index); the LCP scratch overlays the sort's buffers, which are dead by
// then, as in esa_sort (tc_esa_plan.hpp; the carve order here is this build's own), so the one dry run sizes the peak of both.
static tc_fm *fm_build_device(tc_ctx *ctx, const u8 *text_host, u64 n, const u8 *text_dev = nullptr, u32 sa_rate = 1,
                              u32 text_rate = 0, bool with_lcp = false) {
    tc_fm *fm = new tc_fm();
    fm->device = ctx->device;
    fm->n = n;
    fm->N = n + 1;
    fm->sa_rate = sa_rate;
    try {
        const u64 N = n + 1;
        hipStream_t s = ctx->stream;
        const bool sampled = sa_rate > 1;
        TC_HIP(ctx, hipMalloc((void **)&fm->d_L, N + 16));
        if (!sampled) TC_HIP(ctx, hipMalloc((void **)&fm->d_sa, N * sizeof(u32)));
        TC_HIP(ctx, hipMalloc((void **)&fm->d_tab, 768 * sizeof(u32)));
        u8 *d_text = nullptr;
        u32 *d_sa = fm->d_sa;
        MinTree tree;
        LcpScratch lcp_ws;
        if (with_lcp) {
            tree.shape(ctx, (u32)N);
            fm->lcp_fan_log2 = tree.lf;
            fm->lmin_words = tree.words;
            TC_HIP(ctx, hipMalloc((void **)&fm->d_lcp, N * sizeof(u32)));
            TC_HIP(ctx, hipMalloc((void **)&fm->d_lmin, (size_t)tree.words * sizeof(u32)));
        }
        auto plan = [&](Arena &A, bool dry) {
            if (sampled) d_sa = esa_sa_arg(A.get<u32>(N), dry);
            if (text_dev) {
                d_text = const_cast<u8 *>(text_dev);
            } else {
                d_text = A.get<u8>(n + 16);
                if (!dry) tc_h2d(ctx, d_text, text_host, n);
            }
            const size_t mark = A.off;
            sa_build(ctx, A, d_text, n, d_sa, fm->d_L, &fm->primary, fm->counts, dry);
            if (with_lcp) {
                A.rewind(mark);
                lcp_ws.carve(ctx, A, n);
            }
        };
        ctx->stats = tc_stats{};
        ctx->stats.n = n; ctx->stats.N = N;
        tc_ws_plan(ctx, 0, plan);
        if (with_lcp) {
            lcp_device(ctx, lcp_ws, d_text, n, d_sa, fm->d_lcp);
            tree.build(ctx, fm->d_lcp, fm->d_lmin);
        }
        // C[c] = #symbols of text.'$' smaller than c ('$' = Nothing counts once)
        u32 tab[768];
        const u32 sig = fm_make_tab(fm->counts, tab, fm->sym_of_code);
        fm->sigma_bytes = sig;
        fm->lines = N / FM_LINE_BITS + 1;
        TC_HIP(ctx, hipMalloc((void **)&fm->d_bits, (size_t)sig * fm->lines * 64));
        tc_h2d(ctx, fm->d_tab, tab, sizeof tab);
        TC_HIP(ctx, hipStreamSynchronize(s));  // tab is a stack buffer
        fm_bits_kernel<<<tc_cdiv(fm->lines, 4), 256, 0, s>>>(fm->d_L, N, fm->primary, fm->d_tab, sig,
                                                            fm->lines, fm->d_bits);
        TC_LAUNCH_CHECK(ctx);
        fm_scan_kernel<<<sig, 1024, 0, s>>>(fm->d_bits, fm->lines);
        TC_LAUNCH_CHECK(ctx);
        if (sig <= FM_PAIR_SIGMA && n >= 2 && env_int("TC_FM_PAIRS", 1) != 0) {
            TC_HIP(ctx, hipMalloc((void **)&fm->d_tab2, FM_PAIR_SIGMA * FM_PAIR_SIGMA * sizeof(u32)));
            fm_alloc_bits2(ctx, fm, (size_t)sig * sig * fm->lines * 64);
            TC_HIP(ctx, hipMemsetAsync(fm->d_tab2, 0, FM_PAIR_SIGMA * FM_PAIR_SIGMA * sizeof(u32), s));
            fm_bits2_kernel<<<tc_cdiv(fm->lines, 4), 256, 0, s>>>(fm->d_L, d_sa, d_text, N, fm->d_tab, sig,
                                                                 fm->lines, fm->d_bits2);
            TC_LAUNCH_CHECK(ctx);
            fm_scan_kernel<<<sig * sig, 1024, 0, s>>>(fm->d_bits2, fm->lines);
            TC_LAUNCH_CHECK(ctx);
            fm_c2_kernel<<<1, 64, 0, s>>>(fm->d_bits, fm->lines, fm->d_tab, sig, fm->d_tab2);
            TC_LAUNCH_CHECK(ctx);
        }
        if (sampled) {
            fm->nsamples = n / sa_rate + 1;
            TC_HIP(ctx, hipMalloc((void **)&fm->d_marks, (size_t)fm->lines * 64));
            TC_HIP(ctx, hipMalloc((void **)&fm->d_samples, (size_t)fm->nsamples * sizeof(u32)));
            fm_marks_kernel<<<tc_cdiv(fm->lines, 4), 256, 0, s>>>(d_sa, N, sa_rate, fm->lines, fm->d_marks);
            TC_LAUNCH_CHECK(ctx);
            fm_scan_kernel<<<1, 1024, 0, s>>>(fm->d_marks, fm->lines);
            TC_LAUNCH_CHECK(ctx);
            fm_samples_kernel<<<tc_cdiv(fm->lines, 4), 256, 0, s>>>(d_sa, N, fm->lines, fm->d_marks, fm->nsamples,
                                                                   fm->d_samples);
            TC_LAUNCH_CHECK(ctx);
        }
        if (text_rate) {
            fm->text_rate = text_rate;
            fm->nisa = n / text_rate + 1;
            TC_HIP(ctx, hipMalloc((void **)&fm->d_isa, (size_t)fm->nisa * sizeof(u32)));
            u32 grid = tc_cdiv(N, 256 * 8);
            if (grid > 8192) grid = 8192;
            fm_isa_kernel<<<grid, 256, 0, s>>>(d_sa, N, text_rate, fm_log2(text_rate), fm->nisa, fm->d_isa);
            TC_LAUNCH_CHECK(ctx);
        }
        tc_sync_check(ctx);
    } catch (...) {
        fm_release(fm);
        throw;
    }
    return fm;
}

// ranges (device, 2*npat u64) may be null
static void fm_count_device(tc_ctx *ctx, const tc_fm *fm, const u8 *d_pats, const u64 *d_offs,
                            u64 npat, i64 *d_out, u64 *d_ranges) {
    if (fm->d_bits2)
        fm_count_kernel<true><<<tc_cdiv(npat, 256), 256, 0, ctx->stream>>>(fm->d_bits, fm->d_bits2, fm->lines, fm->d_tab,
                                                                           fm->d_tab2, fm->sigma_bytes, fm->N, d_pats,
                                                                           d_offs, npat, d_out, d_ranges);
    else
        fm_count_kernel<false><<<tc_cdiv(npat, 256), 256, 0, ctx->stream>>>(fm->d_bits, nullptr, fm->lines, fm->d_tab,
                                                                            nullptr, fm->sigma_bytes, fm->N, d_pats,
                                                                            d_offs, npat, d_out, d_ranges);
    TC_LAUNCH_CHECK(ctx);
}

// fm_mm_kernel over a batch.  d_hoffs = null: the count pass (d_out[p] = hits of pattern p within distance k).  Otherwise the
// fill pass: the same enumeration writes pattern p's hits to d_hits[d_hoffs[p] .. d_hoffs[p + 1]) -- positions on a full
// index, rows on a sampled one -- and their distances to d_mm (may be null).
static void fm_mm_device(tc_ctx *ctx, const tc_fm *fm, const u8 *d_pats, const u64 *d_offs, u64 npat, u32 k, i64 *d_out,
                         const u64 *d_hoffs, u64 *d_hits, u8 *d_mm) {
    const u32 grid = tc_cdiv(npat, 256);
    hipStream_t s = ctx->stream;
#define FM_MM_LAUNCH(P, F)                                                                                                  \
    fm_mm_kernel<P, F><<<grid, 256, 0, s>>>(fm->d_bits, fm->d_bits2, fm->lines, fm->d_tab, fm->d_tab2, fm->sigma_bytes,      \
                                            (u32)fm->N, k, d_pats, d_offs, npat, d_out, d_hoffs, fm->d_sa, d_hits, d_mm)
    if (d_hoffs) {
        if (fm->d_bits2) FM_MM_LAUNCH(true, true); else FM_MM_LAUNCH(false, true);
    } else {
        if (fm->d_bits2) FM_MM_LAUNCH(true, false); else FM_MM_LAUNCH(false, false);
    }
#undef FM_MM_LAUNCH
    TC_LAUNCH_CHECK(ctx);
}

// ======================================================================================================================
// The bodies of the tc_fm_* entry points (textcomp.hip forwards to them inside TC_API_BEGIN / TC_API_END).  A pair of
// entry points that differs only in where its buffers live is one function with a `dev` flag; the exact search and the
// search with mismatches are one function with an `exact` flag (k is ignored when it is set).

static_assert(TC_FM_MAX_MISMATCH == FM_MM_MAXK, "fm_mm_kernel keeps TC_FM_MAX_MISMATCH frames per lane");

static inline bool fm_rate_ok(u32 r) { return r >= 1 && r <= TC_FM_MAX_SA_RATE && (r & (r - 1)) == 0; }

// the index of an empty text (FMIndex.hs:366: every query returns the empty result), and what an import starts from
static tc_fm *fm_new_empty(tc_ctx *ctx) {
    tc_fm *fm = new tc_fm();
    fm->device = ctx->device;
    return fm;
}

// the eight tc_fm_build*: text_host or text_dev is the text (the other is null); rates = how many of (sa_rate, text_rate) are
// the caller's and therefore validated -- 0: tc_fm_build, 1: tc_fm_build_sampled, 2: tc_fm_build_self and tc_fm_build_lcp
// (lcp: with the LCP part; there text_rate may also be 0, no text samples)
static void fm_build_entry(tc_ctx *ctx, const u8 *text_host, const u8 *text_dev, u64 n, u32 sa_rate, u32 text_rate, int rates,
                           tc_fm **out, bool lcp = false) {
    static const char *const kBadArg[3] = {"bad argument", "bad argument (sa_rate: a power of two, 1 .. %d)",
                                           "bad argument (sa_rate, text_rate: powers of two, 1 .. %d)"};
    if (out) *out = nullptr;
    if (!out || n > TC_MAX_N || (rates >= 1 && !fm_rate_ok(sa_rate)) || (rates >= 2 && !fm_rate_ok(text_rate) && !(lcp && text_rate == 0)))
        TC_FAIL(ctx, TC_ERR_ARG, kBadArg[rates], TC_FM_MAX_SA_RATE);
    if (n == 0) {
        *out = fm_new_empty(ctx);
        return;
    }
    if (!text_host && !text_dev) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    *out = fm_build_device(ctx, text_host, n, text_dev, sa_rate, text_rate, lcp);
}

static u64 fm_device_bytes(const tc_fm *fm, int part) {
    if (!fm || fm->n == 0 || part < 0 || part > 3) return 0;
    const u64 ext = fm->text_rate ? fm->nisa * sizeof(u32) : 0;
    if (part == 2) return ext;
    const u64 lcp = fm->d_lcp ? (fm->N + fm->lmin_words) * sizeof(u32) : 0;
    if (part == 3) return lcp;
    u64 loc = 0;
    if (fm->sa_rate == 1) loc = (fm->N + 16) + fm->N * sizeof(u32);
    else if (fm->sa_rate > 1) loc = (fm->N + 16) + fm->lines * 64 + fm->nsamples * sizeof(u32);
    if (part == 1) return loc;
    u64 b = loc + ext + lcp + 768 * sizeof(u32) + (u64)fm->sigma_bytes * fm->lines * 64;
    if (fm->d_bits2) b += (u64)fm->sigma_bytes * fm->sigma_bytes * fm->lines * 64 + FM_PAIR_SIGMA * FM_PAIR_SIGMA * sizeof(u32);
    return b;
}

static int fm_info(const tc_fm *fm, u64 *N, u32 *sigma, i16 *c_sym, u64 *c_val, u64 *primary) {
    if (!fm) return TC_ERR_ARG;
    if (N) *N = fm->N;
    if (primary) *primary = fm->primary;
    u32 sg = 0;
    if (fm->n) {  // seqToCc rows: (0, Nothing) first, then every present byte
        u64 acc = 1;
        if (c_sym) c_sym[0] = -1;
        if (c_val) c_val[0] = 0;
        sg = 1;
        for (u32 c = 0; c < fm->sigma_bytes; c++, sg++) {
            if (c_sym) c_sym[sg] = fm->sym_of_code[c];
            if (c_val) c_val[sg] = acc;
            acc += fm->counts[fm->sym_of_code[c]];
        }
    }
    if (sigma) *sigma = sg;
    return TC_OK;
}

// ---- the index as one device byte string (replication over the GPUs of a node) ----------------
struct FmWire {
    char magic[8];   // "TCFMI02\0"
    u64 n, N, primary, lines, bytes;
    u32 sigma_bytes, with_locate;   // with_locate: bit 0 = the locate part follows; bits 8.. = text_rate of the text samples
                                    // that follow the locate part (0: none -- an index without them writes 0 or 1 as ever)
    u32 with_pairs, sa_rate;    // 1: the pair vectors (sigma_bytes^2 of them) follow the per-byte vectors.  sa_rate (the word was
                                // reserved = 0 before sampled indexes): 0 or 1 = the locate part is L + the full suffix array;
                                // k > 1 = L + marks + samples (a full index writes 0: its export is what it always was)
    u32 counts[256];
    i16 sym_of_code[256];
};
static const char kFmMagic[8] = {'T', 'C', 'F', 'M', 'I', '0', '2', 0};
static inline u64 fm_wire_align(u64 v) { return (v + 255) & ~(u64)255; }

// What follows the header, in order: every part is `bytes` long and takes `padded` bytes of the string.  This list is the
// layout: the size, the export's copies, the import's size check and the import's copies all walk it.
enum FmPartKind { FM_PART_BITS, FM_PART_BITS2, FM_PART_L, FM_PART_MARKS, FM_PART_SAMPLES, FM_PART_SA, FM_PART_ISA };
enum { FM_LOCATE_NONE = 0, FM_LOCATE_FULL = 1, FM_LOCATE_SAMPLED = 2 };
struct FmWireLayout {
    struct Part {
        FmPartKind kind;
        u64 bytes, padded;
    } part[6];
    int nparts = 0;
    u64 total = fm_wire_align(sizeof(FmWire));
    void add(FmPartKind kind, u64 bytes, u64 reserved) {
        part[nparts++] = {kind, bytes, fm_wire_align(reserved)};
        total += fm_wire_align(reserved);
    }
};
static FmWireLayout fm_wire_layout(u64 n, u64 N, u64 lines, u32 sigma_bytes, bool with_pairs, int locate, u64 nsamples, u64 nisa) {
    FmWireLayout Y;
    if (n == 0) return Y;
    const u64 bb = (u64)sigma_bytes * lines * 64;
    Y.add(FM_PART_BITS, bb, bb);
    if (with_pairs) Y.add(FM_PART_BITS2, bb * sigma_bytes, bb * sigma_bytes);
    if (locate) Y.add(FM_PART_L, N, N + 16);
    if (locate == FM_LOCATE_SAMPLED) {
        Y.add(FM_PART_MARKS, lines * 64, lines * 64);
        Y.add(FM_PART_SAMPLES, nsamples * sizeof(u32), nsamples * sizeof(u32));
    } else if (locate) {
        Y.add(FM_PART_SA, N * sizeof(u32), N * sizeof(u32));
    }
    if (nisa) Y.add(FM_PART_ISA, nisa * sizeof(u32), nisa * sizeof(u32));
    return Y;
}
// what an export of fm holds (the text samples travel only behind a locate part)
static FmWireLayout fm_wire_layout(const tc_fm *fm, int with_locate) {
    return fm_wire_layout(fm->n, fm->N, fm->lines, fm->sigma_bytes, fm->d_bits2 != nullptr,
                          !with_locate ? FM_LOCATE_NONE : fm->sa_rate > 1 ? FM_LOCATE_SAMPLED : FM_LOCATE_FULL, fm->nsamples,
                          with_locate && fm->text_rate ? fm->nisa : 0);
}
// the index's device pointer of a part
static void **fm_part_slot(tc_fm *fm, FmPartKind kind) {
    switch (kind) {
    case FM_PART_BITS: return (void **)&fm->d_bits;
    case FM_PART_BITS2: return (void **)&fm->d_bits2;
    case FM_PART_L: return (void **)&fm->d_L;
    case FM_PART_MARKS: return (void **)&fm->d_marks;
    case FM_PART_SAMPLES: return (void **)&fm->d_samples;
    case FM_PART_SA: return (void **)&fm->d_sa;
    default: return (void **)&fm->d_isa;
    }
}

static u64 fm_export_bound(const tc_fm *fm, int with_locate) { return fm ? fm_wire_layout(fm, with_locate).total : 0; }

static void fm_export_device(tc_ctx *ctx, const tc_fm *fm, int with_locate, u8 *d_out, u64 *bytes) {
    if (!fm || !bytes) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const FmWireLayout Y = fm_wire_layout(fm, with_locate);
    const u64 need = Y.total, cap = *bytes;
    *bytes = need;
    if (cap < need) TC_FAIL(ctx, TC_ERR_CAPACITY, "index export needs %llu bytes, have %llu", (unsigned long long)need, (unsigned long long)cap);
    if (!d_out || ((uintptr_t)d_out & 15)) TC_FAIL(ctx, TC_ERR_ARG, "export buffer must be 16-byte aligned");
    FmWire h = {};
    memcpy(h.magic, kFmMagic, 8);
    h.n = fm->n; h.N = fm->N; h.primary = fm->primary; h.lines = fm->lines; h.bytes = need;
    h.sigma_bytes = fm->sigma_bytes; h.with_locate = (fm->n && with_locate) ? (1u | fm->text_rate << 8) : 0u;
    h.with_pairs = fm->d_bits2 ? 1u : 0u;
    h.sa_rate = (h.with_locate && fm->sa_rate > 1) ? fm->sa_rate : 0u;
    memcpy(h.counts, fm->counts, sizeof h.counts);
    memcpy(h.sym_of_code, fm->sym_of_code, sizeof h.sym_of_code);
    hipStream_t s = ctx->stream;
    TC_HIP(ctx, hipMemcpyAsync(d_out, &h, sizeof h, hipMemcpyHostToDevice, s));
    u64 o = fm_wire_align(sizeof(FmWire));
    for (int i = 0; i < Y.nparts; o += Y.part[i++].padded)
        TC_HIP(ctx, hipMemcpyAsync(d_out + o, *fm_part_slot(const_cast<tc_fm *>(fm), Y.part[i].kind), Y.part[i].bytes,
                                   hipMemcpyDeviceToDevice, s));
    TC_HIP(ctx, hipStreamSynchronize(s));   // h is a stack object
}

// an import check only the device can make: `launch(grid, d_res)` reduces `items` items into the zeroed 8 bytes at d_res,
// which are returned
template <class Launch>
static u64 fm_import_probe(tc_ctx *ctx, u64 items, Launch &&launch) {
    hipStream_t s = ctx->stream;
    u64 *d_res = ctx->d_scalars + 10;
    TC_HIP(ctx, hipMemsetAsync(d_res, 0, sizeof(u64), s));
    u32 grid = tc_cdiv(items, 256 * 16);
    if (grid > 4096) grid = 4096;
    launch(grid, d_res);
    TC_LAUNCH_CHECK(ctx);
    TC_HIP(ctx, hipMemcpyAsync(&ctx->h_scalars[10], d_res, sizeof(u64), hipMemcpyDeviceToHost, s));
    TC_HIP(ctx, hipStreamSynchronize(s));
    return ctx->h_scalars[10];
}

static void fm_import_device(tc_ctx *ctx, const u8 *d_in, u64 bytes, tc_fm **out) {
    if (!out || !d_in || bytes < sizeof(FmWire)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    *out = nullptr;
    FmWire h;
    hipStream_t s = ctx->stream;
    TC_HIP(ctx, hipMemcpyAsync(&h, d_in, sizeof h, hipMemcpyDeviceToHost, s));
    TC_HIP(ctx, hipStreamSynchronize(s));
    if (memcmp(h.magic, "TCFMI0", 6) == 0 && memcmp(h.magic, kFmMagic, 8) != 0)   // (an export of another build: the layout changed)
        TC_FAIL(ctx, TC_ERR_MALFORMED, "unsupported FM export version %.7s (this build reads %s: an export travels between ranks of one build, it is not an archive format)", h.magic, kFmMagic);
    if (memcmp(h.magic, kFmMagic, 8) != 0 || h.bytes > bytes || h.N != (h.n ? h.n + 1 : 0) || h.n > TC_MAX_N ||
        h.sigma_bytes > 256 || (h.n && h.lines != h.N / FM_LINE_BITS + 1))
        TC_FAIL(ctx, TC_ERR_MALFORMED, "not an exported FM-index");
    {   // the scalars fm_count / fm_locate index with: primary row, symbol counts, code table
        u64 total = 0;
        u32 present = 0;
        bool codes_ok = true;
        for (int b = 0; b < 256; b++) {
            total += h.counts[b];
            if (h.counts[b]) {
                codes_ok = codes_ok && present < h.sigma_bytes && h.sym_of_code[present] == (i16)b;
                present++;
            }
        }
        if (h.n && (h.primary == 0 || h.primary >= h.N || total != h.n || present != h.sigma_bytes || !codes_ok))
            TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: header is inconsistent");
    }
    if (h.with_pairs > 1 || (h.with_pairs && (h.sigma_bytes > FM_PAIR_SIGMA || h.n < 2)))
        TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: header is inconsistent");
    // the sampling rate rides in the word that was reserved: 0 or 1 = full suffix array; otherwise a power of two within range,
    // and only where there is a locate part
    // the text samples' rate rides above bit 7 of the with_locate word: 0 = none; otherwise a power of two within range, and
    // only behind a locate part
    const bool wire_locate = (h.with_locate & 0xffu) != 0;
    const u32 wire_text_rate = h.with_locate >> 8;
    const bool wire_sampled = h.sa_rate > 1;
    if (wire_sampled && (!fm_rate_ok(h.sa_rate) || !wire_locate || !h.n))
        TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: bad suffix-array sampling rate %u", h.sa_rate);
    if (wire_text_rate && (!fm_rate_ok(wire_text_rate) || (h.with_locate & 0xffu) != 1 || !h.n))
        TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: bad text sampling rate %u", wire_text_rate);
    tc_fm *fm = fm_new_empty(ctx);
    fm->n = h.n; fm->N = h.N; fm->primary = h.primary; fm->lines = h.lines; fm->sigma_bytes = h.sigma_bytes;
    memcpy(fm->counts, h.counts, sizeof h.counts);
    memcpy(fm->sym_of_code, h.sym_of_code, sizeof h.sym_of_code);
    try {
        if (fm->n) {
            if (wire_sampled) fm->nsamples = fm->n / h.sa_rate + 1;
            if (wire_text_rate) fm->nisa = fm->n / wire_text_rate + 1;
            const FmWireLayout Y = fm_wire_layout(fm->n, fm->N, fm->lines, fm->sigma_bytes, h.with_pairs != 0,
                                                  wire_sampled ? FM_LOCATE_SAMPLED : wire_locate ? FM_LOCATE_FULL : FM_LOCATE_NONE,
                                                  fm->nsamples, fm->nisa);
            if (Y.total != h.bytes) TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: size mismatch");
            u32 tab[768];
            (void)fm_make_tab(fm->counts, tab, nullptr);
            TC_HIP(ctx, hipMalloc((void **)&fm->d_tab, 768 * sizeof(u32)));
            TC_HIP(ctx, hipMemcpyAsync(fm->d_tab, tab, sizeof tab, hipMemcpyHostToDevice, s));
            TC_HIP(ctx, hipStreamSynchronize(s));   // tab is a stack buffer
            u64 o = fm_wire_align(sizeof(FmWire));
            for (int i = 0; i < Y.nparts; o += Y.part[i++].padded) {
                void **slot = fm_part_slot(fm, Y.part[i].kind);
                const bool is_L = Y.part[i].kind == FM_PART_L;   // (L is allocated with the 16 zero bytes of slack it is exported with)
                TC_HIP(ctx, hipMalloc(slot, Y.part[i].bytes + (is_L ? 16 : 0)));
                if (is_L) TC_HIP(ctx, hipMemsetAsync(fm->d_L + fm->N, 0, 16, s));
                TC_HIP(ctx, hipMemcpyAsync(*slot, d_in + o, Y.part[i].bytes, hipMemcpyDeviceToDevice, s));
            }
            if (h.with_pairs) {
                TC_HIP(ctx, hipMalloc((void **)&fm->d_tab2, FM_PAIR_SIGMA * FM_PAIR_SIGMA * sizeof(u32)));
                TC_HIP(ctx, hipMemsetAsync(fm->d_tab2, 0, FM_PAIR_SIGMA * FM_PAIR_SIGMA * sizeof(u32), s));
                fm_c2_kernel<<<1, 64, 0, s>>>(fm->d_bits, fm->lines, fm->d_tab, fm->sigma_bytes, fm->d_tab2);
                TC_LAUNCH_CHECK(ctx);
            }
            if (wire_sampled) {
                // what only the device can check: the marks hold exactly one bit per sample (the walk bounds everything else)
                const u64 ones = fm_import_probe(ctx, fm->lines * 8, [&](u32 grid, u64 *d_res) {
                    fm_popcount_kernel<<<grid, 256, 0, s>>>(fm->d_marks, fm->lines, reinterpret_cast<unsigned long long *>(d_res));
                });
                if (ones != fm->nsamples)
                    TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: %llu rows are marked as sampled, %llu samples follow",
                            (unsigned long long)ones, (unsigned long long)fm->nsamples);
                fm->sa_rate = h.sa_rate;
            } else if (wire_locate) {
                fm->sa_rate = 1;
            }
            if (wire_text_rate) {
                // what only the device can check: every sample is a row, and position 0 is the primary row's (the walk bounds
                // everything else)
                const u64 res = fm_import_probe(ctx, fm->nisa, [&](u32 grid, u64 *d_res) {
                    fm_isa_max_kernel<<<grid, 256, 0, s>>>(fm->d_isa, fm->nisa, reinterpret_cast<u32 *>(d_res));
                });
                const u64 isa_max = res & 0xffffffffu, isa0 = res >> 32;
                if (isa_max >= fm->N || isa0 != fm->primary)
                    TC_FAIL(ctx, TC_ERR_MALFORMED, "exported FM-index: text samples out of range (largest row %llu of %llu, position 0 at row %llu, primary row %llu)",
                            (unsigned long long)isa_max, (unsigned long long)fm->N, (unsigned long long)isa0, (unsigned long long)fm->primary);
                fm->text_rate = wire_text_rate;
            }
            TC_HIP(ctx, hipStreamSynchronize(s));
        }
    } catch (...) {
        fm_release(fm);
        throw;
    }
    *out = fm;
}

// ---- queries ---------------------------------------------------------------------------------------------------------
// the answer "nothing" of an edge case (an empty index, an empty batch), written where the results live
static void fm_zero_result(tc_ctx *ctx, void *p, size_t bytes, bool dev) {
    if (!dev) {
        memset(p, 0, bytes);
        return;
    }
    tc_memset_async(ctx, p, 0, bytes);
    tc_sync_check(ctx);
}

// the host forms' pattern batch in the workspace: carve inside the call's plan, upload behind it
struct FmPatterns {
    u8 *d_pats = nullptr;
    u64 *d_offs = nullptr;
    void carve(Arena &A, const u64 *offs, u64 npat) {
        d_pats = A.get<u8>(offs[npat] + 16);
        d_offs = A.get<u64>(npat + 1);
    }
    void upload(tc_ctx *ctx, const u8 *pats, const u64 *offs, u64 npat) {
        tc_h2d(ctx, d_pats, pats, offs[npat]);
        tc_h2d(ctx, d_offs, offs, (npat + 1) * sizeof(u64));
    }
};

// the count pass of both searches: d_cnt[p] = hits of pattern p (exactly, or within distance k); d_ranges (the exact search
// only; may be null) as fm_count_kernel writes them
static void fm_count_pass(tc_ctx *ctx, const tc_fm *fm, const u8 *d_pats, const u64 *d_offs, u64 npat, bool exact, u32 k,
                          i64 *d_cnt, u64 *d_ranges) {
    if (exact) fm_count_device(ctx, fm, d_pats, d_offs, npat, d_cnt, d_ranges);
    else fm_mm_device(ctx, fm, d_pats, d_offs, npat, k, d_cnt, nullptr, nullptr, nullptr);
}

// tc_fm_count, tc_fm_count_dev, tc_fm_count_mm, tc_fm_count_mm_dev
static void fm_count_entry(tc_ctx *ctx, const tc_fm *fm, const u8 *pats, const u64 *offs, u64 npat, bool exact, u32 k, i64 *out,
                           bool dev) {
    if (!fm) TC_FAIL(ctx, TC_ERR_ARG, "null index");
    if (!exact && k > TC_FM_MAX_MISMATCH) TC_FAIL(ctx, TC_ERR_ARG, "k = %u mismatches (at most %d)", k, TC_FM_MAX_MISMATCH);
    if (npat == 0) return;
    if (!pats || !offs || !out) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (fm->n == 0) return fm_zero_result(ctx, out, npat * sizeof(i64), dev);
    if (dev) {
        fm_count_pass(ctx, fm, pats, offs, npat, exact, k, out, nullptr);
    } else {
        FmPatterns P;
        i64 *d_out = nullptr;
        tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
            P.carve(A, offs, npat);
            d_out = A.get<i64>(npat);
        });
        P.upload(ctx, pats, offs, npat);
        fm_count_pass(ctx, fm, P.d_pats, P.d_offs, npat, exact, k, d_out, nullptr);
        tc_d2h(ctx, out, d_out, npat * sizeof(i64));
    }
    tc_sync_check(ctx);
}

// scratch of one locate batch besides patterns and results (the ranges: the exact search only)
struct FmLocateScratch {
    i64 *d_cnt = nullptr;
    u64 *d_ranges = nullptr, *d_len = nullptr, *d_tsum = nullptr;
    void carve(Arena &A, u64 npat, bool exact) {
        d_cnt = A.get<i64>(npat);
        if (exact) d_ranges = A.get<u64>(2 * npat);
        d_len = A.get<u64>(npat + 1);
        d_tsum = A.get<u64>(tc_cdiv(npat, SCAN_TILE) + 2);
    }
};

// between the two passes of locate and of factorize: the counts of the first pass (W.d_cnt) scanned into d_offs[0 .. npat], the
// last entry the total, which is read back and returned
static u64 fm_offsets_of_counts(tc_ctx *ctx, const FmLocateScratch &W, u64 npat, u64 *d_offs) {
    hipStream_t s = ctx->stream;
    fm_cnt_to_u64_kernel<<<tc_cdiv(npat, 256), 256, 0, s>>>(W.d_cnt, npat, W.d_len);
    TC_LAUNCH_CHECK(ctx);
    const u64 *d_total = tc_scan64(ctx, W.d_len, npat, W.d_tsum, d_offs);
    TC_HIP(ctx, hipMemcpyAsync(d_offs + npat, d_total, sizeof(u64), hipMemcpyDeviceToDevice, s));
    tc_d2h(ctx, &ctx->h_scalars[9], d_total, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    return ctx->h_scalars[9];
}

// everything on the device: the count pass, the scan of the counts (d_hoffs[0 .. npat], the last entry the total, which is
// returned), then -- when the total is neither 0 nor above cap -- the fill pass: the exact search copies its ranges' rows out of
// the suffix array (a full index) or writes the rows themselves (a sampled one); the search with mismatches repeats its
// enumeration, writing positions or rows likewise and the distances to d_mm (may be null).  On a sampled index the walk then
// turns rows into positions.  When the total exceeds cap nothing is written to d_hits or d_mm.  The caller synchronises
// (tc_sync_check: the walk's bounds raise the device error word).
static u64 fm_locate_device(tc_ctx *ctx, const tc_fm *fm, const FmLocateScratch &W, const u8 *d_pats, const u64 *d_offs, u64 npat,
                            bool exact, u32 k, u64 *d_hoffs, u64 *d_hits, u8 *d_mm, u64 cap) {
    hipStream_t s = ctx->stream;
    const u32 grid = tc_cdiv(npat, 256);
    fm_count_pass(ctx, fm, d_pats, d_offs, npat, exact, k, W.d_cnt, W.d_ranges);
    const u64 need = fm_offsets_of_counts(ctx, W, npat, d_hoffs);
    if (need > cap || need == 0) return need;
    if (!exact) {
        fm_mm_device(ctx, fm, d_pats, d_offs, npat, k, nullptr, d_hoffs, d_hits, d_mm);
    } else {
        if (fm->sa_rate > 1) fm_locate_rows_kernel<<<grid, 256, 0, s>>>(W.d_ranges, d_hoffs, npat, cap, d_hits);
        else fm_locate_fill_kernel<<<grid, 256, 0, s>>>(W.d_ranges, d_hoffs, fm->d_sa, npat, cap, d_hits);
        TC_LAUNCH_CHECK(ctx);
    }
    if (fm->sa_rate > 1) {
        fm_locate_walk_kernel<<<tc_cdiv(need, 256), 256, 0, s>>>(fm->d_bits, fm->d_marks, fm->lines, fm->d_tab, fm->sigma_bytes,
                                                                fm->d_L, fm->d_samples, fm->nsamples, fm->N, fm->primary,
                                                                fm->sa_rate, need, d_hits, ctx->d_err);
        TC_LAUNCH_CHECK(ctx);
    }
    return need;
}

// tc_fm_locate, tc_fm_locate_dev, tc_fm_locate_mm, tc_fm_locate_mm_dev (hit_mm: the search with mismatches only; may be null)
static void fm_locate_entry(tc_ctx *ctx, const tc_fm *fm, const u8 *pats, const u64 *offs, u64 npat, bool exact, u32 k,
                            u64 *hit_offs, u64 *hits, u8 *hit_mm, u64 *nhits, bool dev) {
    if (!fm || !nhits) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nhits;
    *nhits = 0;
    if (!exact && k > TC_FM_MAX_MISMATCH) TC_FAIL(ctx, TC_ERR_ARG, "k = %u mismatches (at most %d)", k, TC_FM_MAX_MISMATCH);
    if (npat == 0) return;
    if (!pats || !offs || !hit_offs || (!hits && cap)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (fm->n == 0) return fm_zero_result(ctx, hit_offs, (npat + 1) * sizeof(u64), dev);
    if (!fm->sa_rate) TC_FAIL(ctx, TC_ERR_ARG, "this index was imported without its locate part");
    FmLocateScratch W;
    FmPatterns P;
    u64 *d_hoffs = hit_offs, *d_hits = hits;
    u8 *d_mm = hit_mm;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        if (!dev) P.carve(A, offs, npat);
        W.carve(A, npat, exact);
        if (!dev) {
            d_hoffs = A.get<u64>(npat + 1);
            d_hits = A.get<u64>(cap + 1);
            d_mm = hit_mm ? A.get<u8>(cap + 16) : nullptr;
        }
    });
    if (!dev) P.upload(ctx, pats, offs, npat);
    const u64 need = fm_locate_device(ctx, fm, W, dev ? pats : P.d_pats, dev ? offs : P.d_offs, npat, exact, k, d_hoffs, d_hits,
                                      d_mm, cap);
    *nhits = need;
    if (need > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu hit slots, have %llu", (unsigned long long)need, (unsigned long long)cap);
    if (!dev) {
        tc_d2h(ctx, hit_offs, d_hoffs, (npat + 1) * sizeof(u64));
        if (need) tc_d2h(ctx, hits, d_hits, need * sizeof(u64));
        if (need && hit_mm) tc_d2h(ctx, hit_mm, d_mm, need);
    }
    tc_sync_check(ctx);
}

// scratch of one extract batch besides queries and results
struct FmExtractScratch {
    u64 *d_len = nullptr, *d_segs = nullptr, *d_soffs = nullptr, *d_tsum_b = nullptr, *d_tsum_s = nullptr;
    u32 *d_bad = nullptr;
    void carve(Arena &A, u64 nq) {
        const u64 tiles = tc_cdiv(nq, SCAN_TILE);
        d_len = A.get<u64>(nq);
        d_segs = A.get<u64>(nq);
        d_soffs = A.get<u64>(nq + 1);
        d_tsum_b = A.get<u64>(tiles + 2);
        d_tsum_s = A.get<u64>(tiles + 2);
        d_bad = A.get<u32>(2);
    }
};

// everything on the device: the plan (validation, byte and segment counts, their scans: d_out_offs[0 .. nq], the last entry
// the total), then -- after the host has seen the flag and the totals -- the walks.  Returns the byte total; a bad query is
// TC_ERR_ARG, and then, as with a total above cap, nothing is written to d_out.  The caller synchronises (tc_sync_check:
// the walk's bounds raise the device error word).
static u64 fm_extract_device(tc_ctx *ctx, const tc_fm *fm, const FmExtractScratch &W, const u64 *d_starts, const u64 *d_lens,
                             u64 nq, u64 *d_out_offs, u8 *d_out, u64 cap) {
    hipStream_t s = ctx->stream;
    const u32 lg = fm_log2(fm->text_rate);
    TC_HIP(ctx, hipMemsetAsync(W.d_bad, 0, 2 * sizeof(u32), s));
    fm_extract_plan_kernel<<<tc_cdiv(nq, 256), 256, 0, s>>>(d_starts, d_lens, nq, fm->n, lg, W.d_len, W.d_segs, W.d_bad);
    TC_LAUNCH_CHECK(ctx);
    const u64 *d_bytes = tc_scan64(ctx, W.d_len, nq, W.d_tsum_b, d_out_offs);
    const u64 *d_nsegs = tc_scan64(ctx, W.d_segs, nq, W.d_tsum_s, W.d_soffs);
    TC_HIP(ctx, hipMemcpyAsync(d_out_offs + nq, d_bytes, sizeof(u64), hipMemcpyDeviceToDevice, s));
    tc_d2h(ctx, &ctx->h_scalars[9], d_bytes, sizeof(u64));
    tc_d2h(ctx, &ctx->h_scalars[8], d_nsegs, sizeof(u64));
    tc_d2h(ctx, &ctx->h_scalars[10], W.d_bad, sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(s));
    const u64 need = ctx->h_scalars[9], nsegs = ctx->h_scalars[8];
    if ((u32)ctx->h_scalars[10])
        TC_FAIL(ctx, TC_ERR_ARG, "extract: a query lies outside the text (start is 1-based: 1 <= start, start - 1 + len <= %llu)",
                (unsigned long long)fm->n);
    if (need > cap || nsegs == 0) return need;
    fm_extract_walk_kernel<<<tc_cdiv(nsegs, 256), 256, 0, s>>>(fm->d_bits, fm->lines, fm->d_tab, fm->sigma_bytes, fm->d_L,
                                                             fm->d_isa, fm->nisa, fm->N, fm->primary, lg, d_starts, d_lens,
                                                             W.d_soffs, d_out_offs, nq, nsegs, d_out, ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
    return need;
}

// tc_fm_extract, tc_fm_extract_dev
static void fm_extract_entry(tc_ctx *ctx, const tc_fm *fm, const u64 *starts, const u64 *lens, u64 nq, u64 *out_offs, u8 *out,
                             u64 *nbytes, bool dev) {
    if (!fm || !nbytes) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nbytes;
    *nbytes = 0;
    if (nq == 0) {
        if (out_offs) fm_zero_result(ctx, out_offs, sizeof(u64), dev);
        return;
    }
    if (!fm->text_rate) TC_FAIL(ctx, TC_ERR_ARG, "this index holds no text samples (build it with tc_fm_build_self; an import without the locate part has none)");
    if (!starts || !lens || !out_offs || (!out && cap)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u64 *u_starts = nullptr, *u_lens = nullptr;   // the host form's copies of the queries
    u64 *d_offs = out_offs;
    u8 *d_out = out;
    FmExtractScratch W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        if (!dev) {
            u_starts = A.get<u64>(nq);
            u_lens = A.get<u64>(nq);
            d_offs = A.get<u64>(nq + 1);
        }
        W.carve(A, nq);
        if (!dev) d_out = A.get<u8>(cap + 16);
    });
    if (!dev) {
        tc_h2d(ctx, u_starts, starts, nq * sizeof(u64));
        tc_h2d(ctx, u_lens, lens, nq * sizeof(u64));
    }
    const u64 need = fm_extract_device(ctx, fm, W, dev ? starts : u_starts, dev ? lens : u_lens, nq, d_offs, d_out, cap);
    *nbytes = need;
    if (need > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu bytes, have %llu", (unsigned long long)need, (unsigned long long)cap);
    if (!dev) {
        tc_d2h(ctx, out_offs, d_offs, (nq + 1) * sizeof(u64));
        if (need) tc_d2h(ctx, out, d_out, need);
    }
    tc_sync_check(ctx);
}

// ---- factorize / unfactorize (the kernels: tc_fm_factor.hpp) ---------------------------------------------------------------
// fm_factor_kernel over a batch.  d_foffs = null: the sizes pass (d_cnt[p] = factors of pattern p).  Otherwise the fill pass:
// the same parse writes pattern p's factors to [d_foffs[p], d_foffs[p + 1]) of d_fpos / d_flen -- positions on a full index,
// rows on a sampled one.  (An empty index has no tables: every byte is a literal.)
static void fm_factor_pass(tc_ctx *ctx, const tc_fm *fm, const u8 *d_pats, const u64 *d_offs, u64 npat, i64 *d_cnt,
                           const u64 *d_foffs, u64 *d_fpos, u32 *d_flen) {
    const u32 grid = tc_cdiv(npat, 256);
    hipStream_t s = ctx->stream;
#define FM_FACTOR_LAUNCH(P, F)                                                                                                \
    fm_factor_kernel<P, F><<<grid, 256, 0, s>>>(fm->d_bits, fm->d_bits2, fm->lines, fm->d_tab, fm->d_tab2, fm->sigma_bytes,    \
                                                (u32)fm->N, d_pats, d_offs, npat, d_cnt, d_foffs, fm->d_sa, d_fpos, d_flen)
    if (d_foffs) {
        if (fm->d_bits2) FM_FACTOR_LAUNCH(true, true); else FM_FACTOR_LAUNCH(false, true);
    } else {
        if (fm->d_bits2) FM_FACTOR_LAUNCH(true, false); else FM_FACTOR_LAUNCH(false, false);
    }
#undef FM_FACTOR_LAUNCH
    TC_LAUNCH_CHECK(ctx);
}

// everything on the device: the sizes pass, the scan of the counts (d_foffs[0 .. npat], the last entry the total, which is
// returned), then -- when the total is neither 0 nor above cap -- the fill pass and, on a sampled index, the walk that turns
// the match factors' rows into positions.  When the total exceeds cap nothing is written to d_fpos or d_flen.  The caller
// synchronises (tc_sync_check: the walk's bounds raise the device error word).
static u64 fm_factor_device(tc_ctx *ctx, const tc_fm *fm, const FmLocateScratch &W, const u8 *d_pats, const u64 *d_offs, u64 npat,
                            u64 *d_foffs, u64 *d_fpos, u32 *d_flen, u64 cap) {
    fm_factor_pass(ctx, fm, d_pats, d_offs, npat, W.d_cnt, nullptr, nullptr, nullptr);
    const u64 need = fm_offsets_of_counts(ctx, W, npat, d_foffs);
    if (need > cap || need == 0) return need;
    fm_factor_pass(ctx, fm, d_pats, d_offs, npat, nullptr, d_foffs, d_fpos, d_flen);
    if (fm->sa_rate > 1) {
        fm_factor_walk_kernel<<<tc_cdiv(need, 256), 256, 0, ctx->stream>>>(fm->d_bits, fm->d_marks, fm->lines, fm->d_tab,
                                                                          fm->sigma_bytes, fm->d_L, fm->d_samples, fm->nsamples,
                                                                          fm->N, fm->primary, fm->sa_rate, need, d_fpos, d_flen,
                                                                          ctx->d_err);
        TC_LAUNCH_CHECK(ctx);
    }
    return need;
}

// tc_fm_factorize, tc_fm_factorize_dev.  fac_pos = fac_len = null with capacity 0 is the sizes-only form: fac_offs and the
// total, TC_OK.
static void fm_factor_entry(tc_ctx *ctx, const tc_fm *fm, const u8 *pats, const u64 *offs, u64 npat, u64 *fac_offs, u64 *fac_pos,
                            u32 *fac_len, u64 *nfac, bool dev) {
    if (!fm || !nfac) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nfac;
    *nfac = 0;
    if (npat == 0) return;
    const bool sizes_only = !fac_pos && !fac_len && cap == 0;
    if (!pats || !offs || !fac_offs || (!sizes_only && (!fac_pos || !fac_len))) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (fm->n && !fm->sa_rate) TC_FAIL(ctx, TC_ERR_ARG, "this index was imported without its locate part");
    FmLocateScratch W;
    FmPatterns P;
    u64 *d_foffs = fac_offs, *d_fpos = fac_pos;
    u32 *d_flen = fac_len;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        if (!dev) P.carve(A, offs, npat);
        W.carve(A, npat, false);
        if (!dev) {
            d_foffs = A.get<u64>(npat + 1);
            d_fpos = A.get<u64>(cap + 1);
            d_flen = A.get<u32>(cap + 1);
        }
    });
    if (!dev) P.upload(ctx, pats, offs, npat);
    const u64 need = fm_factor_device(ctx, fm, W, dev ? pats : P.d_pats, dev ? offs : P.d_offs, npat, d_foffs, d_fpos, d_flen,
                                      sizes_only ? 0 : cap);
    *nfac = need;
    if (!dev) tc_d2h(ctx, fac_offs, d_foffs, (npat + 1) * sizeof(u64));
    if (need > cap && !sizes_only) {
        tc_sync_check(ctx);
        TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu factor slots, have %llu", (unsigned long long)need, (unsigned long long)cap);
    }
    if (!dev && need && !sizes_only) {
        tc_d2h(ctx, fac_pos, d_fpos, need * sizeof(u64));
        tc_d2h(ctx, fac_len, d_flen, need * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// scratch of one unfactorize batch besides factors and results: that of a flat extract over nf factors, the factors' byte
// offsets [nf + 1] (what the extract calls out_offs), and the factor lengths as the walk reads them (FmExtractScratch::d_len)
struct FmUnfactorScratch {
    FmExtractScratch X;
    u64 *d_boffs = nullptr;
    void carve(Arena &A, u64 nf) {
        X.carve(A, nf ? nf : 1);
        d_boffs = A.get<u64>(nf + 1);
    }
};

// everything on the device, nf = the factor total (fac_offs[npat], read by the entry): the offsets' check and the plan
// (validation, byte and segment counts, their scans), the gather of d_out_offs[0 .. npat], then -- after the host has seen
// the flag and the totals -- fm_extract_walk_kernel, unchanged, over the match factors (a factor is a query (pos, len); the
// walk never selects a factor without segments) and the literals' bytes.  Returns the byte total; a bad list is TC_ERR_ARG,
// and then, as with a total above cap, nothing is written to d_out.  The caller synchronises.
static u64 fm_unfactor_device(tc_ctx *ctx, const tc_fm *fm, const FmUnfactorScratch &W, const u64 *d_foffs, const u64 *d_fpos,
                              const u32 *d_flen, u64 npat, u64 nf, u64 *d_out_offs, u8 *d_out, u64 cap) {
    hipStream_t s = ctx->stream;
    const u32 lg = fm_log2(fm->text_rate);
    const FmExtractScratch &X = W.X;
    TC_HIP(ctx, hipMemsetAsync(X.d_bad, 0, 2 * sizeof(u32), s));
    TC_HIP(ctx, hipMemsetAsync(W.d_boffs, 0, sizeof(u64), s));
    fm_unfactor_offs_kernel<<<tc_cdiv(npat, 256), 256, 0, s>>>(d_foffs, npat, X.d_bad);
    TC_LAUNCH_CHECK(ctx);
    u64 need = 0, nsegs = 0;
    if (nf) {
        fm_unfactor_plan_kernel<<<tc_cdiv(nf, 256), 256, 0, s>>>(d_fpos, d_flen, nf, fm->n, lg, X.d_len, X.d_segs, X.d_bad);
        TC_LAUNCH_CHECK(ctx);
        const u64 *d_bytes = tc_scan64(ctx, X.d_len, nf, X.d_tsum_b, W.d_boffs);
        const u64 *d_nsegs = tc_scan64(ctx, X.d_segs, nf, X.d_tsum_s, X.d_soffs);
        TC_HIP(ctx, hipMemcpyAsync(W.d_boffs + nf, d_bytes, sizeof(u64), hipMemcpyDeviceToDevice, s));
        tc_d2h(ctx, &ctx->h_scalars[9], d_bytes, sizeof(u64));
        tc_d2h(ctx, &ctx->h_scalars[8], d_nsegs, sizeof(u64));
    }
    tc_d2h(ctx, &ctx->h_scalars[10], X.d_bad, sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(s));
    if (nf) need = ctx->h_scalars[9], nsegs = ctx->h_scalars[8];
    if ((u32)ctx->h_scalars[10])
        TC_FAIL(ctx, TC_ERR_ARG, "unfactorize: a bad factor list (fac_offs starts at 0 and never decreases; a match has 1 <= pos, pos - 1 + len <= %llu; a literal has len 0 and pos <= 255)",
                (unsigned long long)fm->n);
    fm_unfactor_gather_kernel<<<tc_cdiv(npat + 1, 256), 256, 0, s>>>(d_foffs, npat, W.d_boffs, d_out_offs);
    TC_LAUNCH_CHECK(ctx);
    if (need > cap || need == 0) return need;
    if (nsegs) {
        fm_extract_walk_kernel<<<tc_cdiv(nsegs, 256), 256, 0, s>>>(fm->d_bits, fm->lines, fm->d_tab, fm->sigma_bytes, fm->d_L,
                                                                 fm->d_isa, fm->nisa, fm->N, fm->primary, lg, d_fpos, X.d_len,
                                                                 X.d_soffs, W.d_boffs, nf, nsegs, d_out, ctx->d_err);
        TC_LAUNCH_CHECK(ctx);
    }
    fm_unfactor_literal_kernel<<<tc_cdiv(nf, 256), 256, 0, s>>>(d_fpos, d_flen, nf, W.d_boffs, d_out);
    TC_LAUNCH_CHECK(ctx);
    return need;
}

// tc_fm_unfactorize, tc_fm_unfactorize_dev
static void fm_unfactor_entry(tc_ctx *ctx, const tc_fm *fm, const u64 *fac_offs, const u64 *fac_pos, const u32 *fac_len, u64 npat,
                              u64 *out_offs, u8 *out, u64 *nbytes, bool dev) {
    if (!fm || !nbytes) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nbytes;
    *nbytes = 0;
    if (npat == 0) {
        if (out_offs) fm_zero_result(ctx, out_offs, sizeof(u64), dev);
        return;
    }
    if (!fm->text_rate) TC_FAIL(ctx, TC_ERR_ARG, "this index holds no text samples (build it with tc_fm_build_self; an import without the locate part has none)");
    if (!fac_offs || !out_offs || (!out && cap)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u64 ends[2];    // fac_offs[0] and fac_offs[npat]: the list starts at 0, and its last offset is the factor total
    if (dev) {
        tc_d2h(ctx, &ctx->h_scalars[8], fac_offs, sizeof(u64));
        tc_d2h(ctx, &ctx->h_scalars[9], fac_offs + npat, sizeof(u64));
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ends[0] = ctx->h_scalars[8];
        ends[1] = ctx->h_scalars[9];
    } else {
        ends[0] = fac_offs[0];
        ends[1] = fac_offs[npat];
    }
    const u64 nf = ends[1];
    // (a total no pair of factor arrays can hold is refused here: the sizes below are computed from it)
    if (ends[0] != 0 || nf > ((u64)1 << 40)) TC_FAIL(ctx, TC_ERR_ARG, "unfactorize: a bad factor list (fac_offs[0] = %llu, fac_offs[npat] = %llu)", (unsigned long long)ends[0], (unsigned long long)nf);
    if (nf && (!fac_pos || !fac_len)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u64 *u_foffs = nullptr, *u_fpos = nullptr;   // the host form's copies of the factor list
    u32 *u_flen = nullptr;
    u64 *d_offs = out_offs;
    u8 *d_out = out;
    FmUnfactorScratch W;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        if (!dev) {
            u_foffs = A.get<u64>(npat + 1);
            u_fpos = A.get<u64>(nf + 1);
            u_flen = A.get<u32>(nf + 1);
            d_offs = A.get<u64>(npat + 1);
        }
        W.carve(A, nf);
        if (!dev) d_out = A.get<u8>(cap + 16);
    });
    if (!dev) {
        tc_h2d(ctx, u_foffs, fac_offs, (npat + 1) * sizeof(u64));
        if (nf) tc_h2d(ctx, u_fpos, fac_pos, nf * sizeof(u64));
        if (nf) tc_h2d(ctx, u_flen, fac_len, nf * sizeof(u32));
    }
    const u64 need = fm_unfactor_device(ctx, fm, W, dev ? fac_offs : u_foffs, dev ? fac_pos : u_fpos, dev ? fac_len : u_flen, npat,
                                        nf, d_offs, d_out, cap);
    *nbytes = need;
    if (!dev) tc_d2h(ctx, out_offs, d_offs, (npat + 1) * sizeof(u64));
    if (need > cap) {
        tc_sync_check(ctx);
        TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu bytes, have %llu", (unsigned long long)need, (unsigned long long)cap);
    }
    if (!dev && need) tc_d2h(ctx, out, d_out, need);
    tc_sync_check(ctx);
}

// ---- matching statistics / maximal exact matches (the kernels: tc_fm_ms.hpp) ----------------------------------------------
// the number of pattern bytes of a batch, offs[npat] (the result arrays of the matching statistics have that many entries)
static u64 fm_pattern_bytes(tc_ctx *ctx, const u64 *offs, u64 npat, bool dev) {
    if (!dev) return offs[npat];
    tc_d2h(ctx, &ctx->h_scalars[8], offs + npat, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ctx->h_scalars[8];
}

// fm_ms_kernel over a batch: d_len[offs[p] + i] for every position of every pattern, and d_pos / d_occ likewise where they
// are not null -- d_pos holds positions on a full index, rows on a sampled one (the caller walks what it keeps)
static void fm_ms_pass(tc_ctx *ctx, const tc_fm *fm, const u8 *d_pats, const u64 *d_offs, u64 npat, u32 *d_len, u64 *d_pos,
                       u32 *d_occ) {
    const u32 grid = tc_cdiv(npat, 256);
    hipStream_t s = ctx->stream;
#define FM_MS_LAUNCH(P)                                                                                                     \
    fm_ms_kernel<P><<<grid, 256, 0, s>>>(fm->d_bits, fm->lines, fm->d_tab, (u32)fm->N, fm->d_lcp, fm->d_lmin, fm->lcp_fan_log2, \
                                         fm->d_sa, d_pats, d_offs, npat, d_len, d_pos, d_occ)
    if (d_pos || d_occ) FM_MS_LAUNCH(true); else FM_MS_LAUNCH(false);
#undef FM_MS_LAUNCH
    TC_LAUNCH_CHECK(ctx);
}

// the walk of a sampled index over `total` (row, length) entries: rows of entries with length > 0 become positions
static void fm_rows_to_positions(tc_ctx *ctx, const tc_fm *fm, u64 total, u64 *d_pos, const u32 *d_len) {
    fm_factor_walk_kernel<<<tc_cdiv(total, 256), 256, 0, ctx->stream>>>(fm->d_bits, fm->d_marks, fm->lines, fm->d_tab,
                                                                       fm->sigma_bytes, fm->d_L, fm->d_samples, fm->nsamples,
                                                                       fm->N, fm->primary, fm->sa_rate, total, d_pos, d_len,
                                                                       ctx->d_err);
    TC_LAUNCH_CHECK(ctx);
}

// tc_fm_match_stats, tc_fm_match_stats_dev (ms_pos and ms_occ may each be null)
static void fm_match_stats_entry(tc_ctx *ctx, const tc_fm *fm, const u8 *pats, const u64 *offs, u64 npat, u32 *ms_len,
                                 u64 *ms_pos, u32 *ms_occ, bool dev) {
    if (!fm) TC_FAIL(ctx, TC_ERR_ARG, "null index");
    if (npat == 0) return;
    if (!pats || !offs || !ms_len) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (fm->n && !fm->d_lcp) TC_FAIL(ctx, TC_ERR_ARG, "this index holds no LCP part (build it with tc_fm_build_lcp; an import never has one)");
    const u64 total = fm_pattern_bytes(ctx, offs, npat, dev);
    if (total == 0) return;
    if (fm->n == 0) {
        fm_zero_result(ctx, ms_len, total * sizeof(u32), dev);
        if (ms_pos) fm_zero_result(ctx, ms_pos, total * sizeof(u64), dev);
        if (ms_occ) fm_zero_result(ctx, ms_occ, total * sizeof(u32), dev);
        return;
    }
    FmPatterns P;
    u32 *d_len = ms_len, *d_occ = ms_occ;
    u64 *d_pos = ms_pos;
    if (!dev) {
        tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
            P.carve(A, offs, npat);
            d_len = A.get<u32>(total);
            d_pos = ms_pos ? A.get<u64>(total) : nullptr;
            d_occ = ms_occ ? A.get<u32>(total) : nullptr;
        });
        P.upload(ctx, pats, offs, npat);
    }
    fm_ms_pass(ctx, fm, dev ? pats : P.d_pats, dev ? offs : P.d_offs, npat, d_len, d_pos, d_occ);
    if (d_pos && fm->sa_rate > 1) fm_rows_to_positions(ctx, fm, total, d_pos, d_len);
    if (!dev) {
        tc_d2h(ctx, ms_len, d_len, total * sizeof(u32));
        if (ms_pos) tc_d2h(ctx, ms_pos, d_pos, total * sizeof(u64));
        if (ms_occ) tc_d2h(ctx, ms_occ, d_occ, total * sizeof(u32));
    }
    tc_sync_check(ctx);
}

// tc_fm_mems, tc_fm_mems_dev: the matching statistics into the context's scratch, the MEMs of every pattern counted, the
// scan of the counts (mem_offs[0 .. npat], the last entry the total), the capacity check on the host, the fill and -- on a
// sampled index -- the walk over the MEM list only.  mem_start = mem_pos = mem_len = null with capacity 0 is the sizes-only
// form (the matching statistics are then lengths only).  When the total exceeds the capacity nothing is written to the
// three arrays.
static void fm_mems_entry(tc_ctx *ctx, const tc_fm *fm, const u8 *pats, const u64 *offs, u64 npat, u32 min_len, u64 *mem_offs,
                          u64 *mem_start, u64 *mem_pos, u32 *mem_len, u64 *nmem, bool dev) {
    if (!fm || !nmem) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *nmem;
    *nmem = 0;
    if (min_len == 0) TC_FAIL(ctx, TC_ERR_ARG, "min_len = 0 (a match has at least one byte)");
    if (npat == 0) return;
    const bool sizes_only = !mem_start && !mem_pos && !mem_len && cap == 0;
    if (!pats || !offs || !mem_offs || (!sizes_only && (!mem_start || !mem_pos || !mem_len))) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (fm->n && !fm->d_lcp) TC_FAIL(ctx, TC_ERR_ARG, "this index holds no LCP part (build it with tc_fm_build_lcp; an import never has one)");
    if (fm->n == 0) return fm_zero_result(ctx, mem_offs, (npat + 1) * sizeof(u64), dev);
    const u64 total = fm_pattern_bytes(ctx, offs, npat, dev);
    FmLocateScratch W;
    FmPatterns P;
    u32 *d_mslen = nullptr, *d_mlen = mem_len;
    u64 *d_mspos = nullptr, *d_moffs = mem_offs, *d_mstart = mem_start, *d_mpos = mem_pos;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        if (!dev) P.carve(A, offs, npat);
        W.carve(A, npat, false);
        d_mslen = A.get<u32>(total + 1);
        d_mspos = sizes_only ? nullptr : A.get<u64>(total + 1);
        if (!dev) {
            d_moffs = A.get<u64>(npat + 1);
            d_mstart = A.get<u64>(cap + 1);
            d_mpos = A.get<u64>(cap + 1);
            d_mlen = A.get<u32>(cap + 1);
        }
    });
    if (!dev) P.upload(ctx, pats, offs, npat);
    const u8 *d_pats = dev ? pats : P.d_pats;
    const u64 *d_offs = dev ? offs : P.d_offs;
    hipStream_t s = ctx->stream;
    const u32 grid = tc_cdiv(npat, 256);
    fm_ms_pass(ctx, fm, d_pats, d_offs, npat, d_mslen, d_mspos, nullptr);
    fm_mem_count_kernel<<<grid, 256, 0, s>>>(d_mslen, d_offs, npat, min_len, W.d_cnt);
    TC_LAUNCH_CHECK(ctx);
    const u64 need = fm_offsets_of_counts(ctx, W, npat, d_moffs);
    *nmem = need;
    if (!dev) tc_d2h(ctx, mem_offs, d_moffs, (npat + 1) * sizeof(u64));
    if (need > cap && !sizes_only) {
        tc_sync_check(ctx);
        TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu MEM slots, have %llu", (unsigned long long)need, (unsigned long long)cap);
    }
    if (need && !sizes_only) {
        fm_mem_fill_kernel<<<grid, 256, 0, s>>>(d_mslen, d_mspos, d_offs, npat, min_len, d_moffs, d_mstart, d_mpos, d_mlen);
        TC_LAUNCH_CHECK(ctx);
        if (fm->sa_rate > 1) fm_rows_to_positions(ctx, fm, need, d_mpos, d_mlen);
        if (!dev) {
            tc_d2h(ctx, mem_start, d_mstart, need * sizeof(u64));
            tc_d2h(ctx, mem_pos, d_mpos, need * sizeof(u64));
            tc_d2h(ctx, mem_len, d_mlen, need * sizeof(u32));
        }
    }
    tc_sync_check(ctx);
}
