// tc_ibwt.hpp -- the inverse BWT's device code: the sort of the positions by symbol, the splitter walks (by positions
// and by LF), the ranking of the splitter chain and the copy-out.  Driven by ibwt_device (tc_decode_host.hpp).
//
// Inverse BWT replaces fromBWT (reference BWT.hs:93-104: sort (symbol, position))
// + magicInverseBWT (BWT/Internal.hs:163-200: an n-step dependent pointer chase
//   f <- snd (index ys f) from the Nothing row until it returns to row e).
// On the device:
//   1. stable counting sort of positions by symbol (Nothing first) = one/two radix
//      passes -> spos[d] (the `snd` column of the sorted Seq); the `fst` column is
//      implied by the symbol boundaries C[].
//   2. the chase becomes list ranking: one row per block of S rows is a splitter (its offset in
//      the block is a byte-sum hash of the block number, so that periodic inputs -- whose walks
//      keep a constant row mod S -- cannot miss every splitter);
//      each splitter walks to the next splitter (independent walks, in parallel),
//      the splitter chain is ranked by pointer jumping (log K rounds), then every
//      splitter on row e's chain re-walks its segment writing text bytes at their
//      final offsets.  Works for ANY Seq (Maybe Word8): no Nothing => empty output;
//      a second Nothing met on the chain => TC_ERR_MALFORMED (fromJust, :195).
#pragma once
#include <type_traits>
#include "tc_common.hpp"
#include "tc_mtf.hpp"   // SymAcc, Lut8, Lut16

#ifndef IBWT_S
#define IBWT_S 256  // splitter spacing (rows), a power of two
#endif
#define IBWT_SBITS (IBWT_S == 256 ? 8 : IBWT_S == 512 ? 9 : IBWT_S == 1024 ? 10 : 7)

#ifdef __HIPCC__

// the splitter of block q = r / 256 sits at a HASHED offset (the top bits of q times an odd constant); block 0: row 0.
// (Rounds 1-3: -(byte sum of q) mod 256 -- enough against walks that keep their row mod 256 (periodic text: 211 s for
// 256 MiB before it), but an arithmetic progression in q itself: a walk that advances by a constant 17 rows per step -- the
// rows of N^k x, k = 1, 2, .., of an assembly with 17 gaps lie 17 apart -- shifts its residues by -1 per block exactly as the
// offsets did and missed the splitters for tens of thousands of steps: the 2^28-byte record's walk kernel 38 ms instead of 5.)
__device__ __forceinline__ u32 ibwt_split_off(u32 q) {
    return (q * 0x9E3779B1u) >> (32 - IBWT_SBITS);
}
__device__ __forceinline__ u32 ibwt_split_row(u32 q) { return q * IBWT_S + ibwt_split_off(q); }
__device__ __forceinline__ bool ibwt_is_splitter(u32 r) {
    return (r & (u32)(IBWT_S - 1)) == ibwt_split_off(r >> IBWT_SBITS);
}

template <class Acc>
__global__ __launch_bounds__(256) void ibwt_keys_kernel(Acc acc, u32 N, Lut16 lut,
                                                        u64 *__restrict__ keys) {
    u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j < N) keys[j] = (u64)lut.v[acc(j) + 1];
}

struct CTable {
    u32 c[260];  // c[code] = first sorted row of that code; c[sigma] = N
    i16 sym[260];
    u32 sigma;
};

__device__ __forceinline__ int ibwt_sym_of_row(const u32 *s_c, const i16 *s_sym, u32 sigma, u32 r) {
    // largest code with c[code] <= r
    u32 lo = 0, hi = sigma;  // invariant: c[lo] <= r < c[hi]
    while (hi - lo > 1) {
        u32 mid = (lo + hi) >> 1;
        if (s_c[mid] <= r) lo = mid; else hi = mid;
    }
    return (int)s_sym[lo];
}

// Stable counting sort of the positions by symbol in ONE dedicated pass (sigma <= 256): the keys are
// the symbols themselves, so nothing but the position array is written -- 2 bytes read and 4 written
// per symbol instead of a key-building launch plus a generic (key, value) radix pass (30 bytes).
// Same scheme as radix_pass_kernel: 4096-position tiles from an atomic ticket, wave-striped stable
// ranking through per-wave LDS match masks, per-code decoupled look-back, LDS staging, coalesced
// write-out.  cbase[c] = first sorted row of code c.
#define ISC_NT 256
#define ISC_ITEMS 16
#define ISC_TILE (ISC_NT * ISC_ITEMS)
template <class Acc>
__global__ __launch_bounds__(ISC_NT) void ibwt_scatter_kernel(Acc acc, u32 N, Lut16 lut, CTable ct,
                                                             u32 *__restrict__ spos, u64 *status,
                                                             u32 *ticket, u32 *err) {
    constexpr int NW = ISC_NT / 64;
    __shared__ u32 s_hist[NW * 256];
    __shared__ u64 s_mask[NW * 256];
    __shared__ u32 s_vals[ISC_TILE];
    __shared__ u8 s_dig[ISC_TILE];
    __shared__ u32 s_dbase[256], s_gbase[256];
    __shared__ u16 s_lut[260];
    __shared__ u32 s_scan[NW + 1];
    __shared__ u32 s_tile;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    for (int i = tid; i < 257; i += ISC_NT) s_lut[i] = lut.v[i];
    if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    for (int i = tid; i < NW * 256; i += ISC_NT) {
        s_hist[i] = 0;
        s_mask[i] = 0ull;
    }
    __syncthreads();
    const u32 tile = s_tile;
    const u64 base = (u64)tile * ISC_TILE;
    const u32 valid = (N - base) < (u64)ISC_TILE ? (u32)(N - base) : (u32)ISC_TILE;
    const u32 wofs = w * 64 * ISC_ITEMS;
    u32 *wh = s_hist + w * 256;
    u64 *wm = s_mask + w * 256;
    const u64 mybit = 1ull << l;
    u32 dig[ISC_ITEMS], rnk[ISC_ITEMS];
#pragma unroll
    for (int k = 0; k < ISC_ITEMS; k++) {
        const u32 p = wofs + k * 64 + l;
        const u32 d = p < valid ? (u32)s_lut[acc(base + p) + 1] : 255u;   // pads: last code, last
        dig[k] = d;
        atomicOr((unsigned long long *)&wm[d], (unsigned long long)mybit);
        __builtin_amdgcn_wave_barrier();
        const u64 m = wm[d];
        const u32 old = wh[d];
        const u32 prior = __popcll(m & (mybit - 1ull));
        __builtin_amdgcn_wave_barrier();
        if (prior == 0) {
            wh[d] = old + __popcll(m);
            wm[d] = 0ull;
        }
        __builtin_amdgcn_wave_barrier();
        rnk[k] = old + prior;
    }
    __syncthreads();
    u32 tot = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {   // one owner thread per code (ISC_NT == 256 codes)
        const u32 c = s_hist[i * 256 + tid];
        s_hist[i * 256 + tid] = tot;
        tot += c;
    }
    u32 tot_real = tot;
    if (tid == 255) tot_real = tot - (ISC_TILE - valid);
    u64 *st = status + (u64)tile * 256 + tid;
    lb_store(st, (tile == 0 ? LB_FLAG_INC : LB_FLAG_AGG) | (u64)tot_real);
    u32 dtot;
    const u32 dbase = block_excl_sum<ISC_NT>(tot, s_scan, &dtot);
    s_dbase[tid] = dbase;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ISC_ITEMS; k++) {
        const u32 pos = s_dbase[dig[k]] + wh[dig[k]] + rnk[k];
        s_vals[pos] = (u32)base + wofs + k * 64 + l;
        s_dig[pos] = (u8)dig[k];
    }
    u32 excl = 0;
    if (tile > 0) {
        i64 t = (i64)tile - 1;
        u32 spins = 0;
        for (;;) {
            const u64 sv = lb_load(status + (u64)t * 256 + tid);
            const u32 f = (u32)(sv >> 62);
            if (f == 0) {
                if (++spins > LB_SPIN_LIMIT) {
                    atomicOr(err, 2u);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            excl += (u32)LB_VALUE(sv);
            if (f == 2 || t == 0) break;
            t--;
        }
        lb_store(st, LB_FLAG_INC | (u64)(excl + tot_real));
    }
    s_gbase[tid] = ct.c[tid] + excl - dbase;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ISC_ITEMS; k++) {
        const u32 p = tid + k * ISC_NT;
        if (p < valid) spos[s_gbase[s_dig[p]] + p] = s_vals[p];
    }
}

// Splitter q walks to the next splitter row (independent walks, one per lane) and records what it
// passes: the symbols of its segment go to seg + q * IBWT_SEGCAP, their
// number to seglen[q].  Flags: bit 0 = the segment is longer than IBWT_SEGCAP (listed, re-walked by
// ibwt_walk2_kernel), bit 1 = a Nothing row other than row 0 was met (an error only if the segment
// turns out to lie on the chain of row e).
#define IBWT_SEGCAP (16 * IBWT_S)   // segment lengths are geometric with mean IBWT_S: one in 10^7 is longer
// A record that fills up before a splitter row is met is closed where the walk stands and the walk goes
// on as a NEW splitter (slot K + e, e from the counter `nextra`, at most extra_cap of them): no segment is
// ever walked twice -- a second, serial walk of one long segment costs ~1 us per row, 4 ms for a full
// record, whatever the rest of the grid does.
// The record of one walk's segment, the one place that knows its format: the symbols, sixteen per store, at
// seg + q * IBWT_SEGCAP; the successor, the steps and the symbols passed and the flags in nxt / dist / seglen / segflag [q].
struct SegRecorder {
    u8 *__restrict__ seg;
    u32 *__restrict__ nxt, *__restrict__ dist, *__restrict__ seglen;
    u8 *__restrict__ segflag;
    u32 q;
    u8 *out;
    u32 steps, emitted, flag, word;
    uint4 w4;
    __device__ __forceinline__ void open(u32 slot, u32 fl) {
        q = slot;
        out = seg + (u64)q * IBWT_SEGCAP;
        steps = 0;
        emitted = 0;
        word = 0;
        w4 = make_uint4(0, 0, 0, 0);
        flag = fl;
    }
    __device__ __forceinline__ void keep_word(u32 k4) {
        if (k4 == 0) w4.x = word;
        else if (k4 == 1) w4.y = word;
        else if (k4 == 2) w4.z = word;
        else w4.w = word;
    }
    __device__ __forceinline__ void put(u32 byte) {
        if (emitted < IBWT_SEGCAP) {
            word |= byte << (8 * (emitted & 3u));
            if ((emitted & 3u) == 3u) {   // sixteen symbols per store
                const u32 k4 = (emitted >> 2) & 3u;
                keep_word(k4);
                if (k4 == 3) reinterpret_cast<uint4 *>(out)[emitted >> 4] = w4;
                word = 0;
            }
        } else {
            flag |= 1u;
        }
        emitted++;
    }
    // (a record closed because it is full holds whole groups only: segcap is a multiple of sixteen)
    __device__ __forceinline__ void close(u32 next) {
        if (emitted < IBWT_SEGCAP && (emitted & 15u)) {   // the last, partial group of sixteen
            keep_word((emitted >> 2) & 3u);                 // (so many words of w4 are already complete)
            reinterpret_cast<uint4 *>(out)[emitted >> 4] = w4;
        }
        nxt[q] = next;
        dist[q] = steps;
        seglen[q] = emitted;
        segflag[q] = (u8)flag;
    }
    // record full: close it here, go on as a new splitter
    __device__ __forceinline__ void extend_if_full(u32 K, u32 segcap, u32 *nextra, u32 extra_cap) {
        if (emitted != segcap || !extra_cap) return;
        const u32 e = atomicAdd(nextra, 1u);
        if (e < extra_cap) {
            close(K + e);
            open(K + e, 0);
        }   // (else: slots used up -- the host repeats the walk the old way)
    }
};
__device__ __forceinline__ void ibwt_inert_slot(u32 q, u32 *__restrict__ nxt, u32 *__restrict__ dist,
                                                u32 *__restrict__ seglen, u8 *__restrict__ segflag) {
    nxt[q] = q;
    dist[q] = 0;
    seglen[q] = 0;
    segflag[q] = 0;
}
// Is slot q on row e's chain?  (Ranked, the successor of every slot on it is the terminal, slot 0.)  If so, where its
// segment starts in the walk's output; Lc = the length of row e's cycle.  (Two calls, so that a kernel keeps its own
// tests between them: the loads of the second stay behind those.)
__device__ __forceinline__ bool ibwt_on_chain(u32 q, const u32 *__restrict__ nxt) { return q == 0 || nxt[q] == 0; }
__device__ __forceinline__ u32 ibwt_chain_offset(u32 q, const u32 *__restrict__ dist, const u64 *__restrict__ scalars,
                                                 u32 &Lc) {
    Lc = (u32)scalars[6];
    return (q == 0) ? 0u : Lc - dist[q];
}
__device__ __forceinline__ void ibwt_stage_ctable(const CTable &ct, u32 *s_c, i16 *s_sym) {
    for (int i = threadIdx.x; i < 260; i += 256) {
        s_c[i] = ct.c[i];
        s_sym[i] = ct.sym[i];
    }
    __syncthreads();
}
__global__ __launch_bounds__(256) void ibwt_extra_init_kernel(u32 K, u32 Ktot, u32 *__restrict__ nxt,
                                                              u32 *__restrict__ dist, u32 *__restrict__ seglen,
                                                              u8 *__restrict__ segflag) {
    const u32 q = K + blockIdx.x * 256 + threadIdx.x;
    if (q >= Ktot) return;
    ibwt_inert_slot(q, nxt, dist, seglen, segflag);   // inert until a walk takes the slot
}
__global__ __launch_bounds__(256) void ibwt_walk1_kernel(const u32 *__restrict__ spos, u32 N, u32 K,
                                                         u32 *__restrict__ nxt,
                                                         u32 *__restrict__ dist, CTable ct,
                                                         u8 *__restrict__ seg, u32 *__restrict__ seglen,
                                                         u8 *__restrict__ segflag, u32 force_rewalk,
                                                         u32 *__restrict__ noverflow, u32 *__restrict__ ovlist,
                                                         u32 *__restrict__ nextra, u32 extra_cap, u32 segcap) {
    __shared__ u32 s_c[260];
    __shared__ i16 s_sym[260];
    ibwt_stage_ctable(ct, s_c, s_sym);
    const u32 q = blockIdx.x * 256 + threadIdx.x;
    if (q >= K) return;
    u32 r = ibwt_split_row(q);
    if (r >= N) {  // the last, partial block may not hold its splitter row: inert slot
        ibwt_inert_slot(q, nxt, dist, seglen, segflag);
        return;
    }
    SegRecorder rec{seg, nxt, dist, seglen, segflag};
    rec.open(q, force_rewalk ? 1u : 0u);
    // the load of the NEXT row is issued before this row's symbol is looked up and stored, so the
    // lookup hides behind the (dependent, random) load; the one load past the last row is harmless
    r = spos[r];
    for (;;) {
        rec.steps++;
        const u32 rn = spos[r];
        if (r != 0) {
            const int sym = ibwt_sym_of_row(s_c, s_sym, ct.sigma, r);
            if (sym < 0) rec.flag |= 2u;
            rec.put((u32)(u8)sym);
        }
        if (ibwt_is_splitter(r) || rec.steps > N) break;
        rec.extend_if_full(K, segcap, nextra, extra_cap);
        r = rn;
    }
    rec.close(r / IBWT_S);
    if (rec.flag & 1u) ovlist[atomicAdd(noverflow, 1u)] = rec.q;   // rare: re-walked by ibwt_walk2_kernel
}

// keep splitter 0's real successor aside and make it the terminal of the chain
__global__ void ibwt_terminal_kernel(u32 *nxt, u32 *dist, u64 *scalars) {
    scalars[4] = nxt[0];
    scalars[5] = dist[0];
    nxt[0] = 0;
    dist[0] = 0;
}

__global__ __launch_bounds__(256) void ibwt_jump_kernel(const u32 *__restrict__ nxt,
                                                        const u32 *__restrict__ dist,
                                                        u32 *__restrict__ nxt2,
                                                        u32 *__restrict__ dist2, u32 K) {
    u32 q = blockIdx.x * 256 + threadIdx.x;
    if (q >= K) return;
    u32 n = nxt[q];
    nxt2[q] = nxt[n];
    dist2[q] = dist[q] + dist[n];
}

// Lc = length of row e's cycle; scalars[6] = Lc
__global__ void ibwt_len_kernel(const u32 *nxt, const u32 *dist, u64 *scalars, u32 *err) {
    u32 n0 = (u32)scalars[4], d0 = (u32)scalars[5];
    if (n0 != 0 && nxt[n0] != 0) atomicOr(err, 4u);  // e's chain must come back to e
    scalars[6] = (u64)d0 + (n0 == 0 ? 0u : dist[n0]);
}

// second walk, only for on-chain segments that did not fit their buffer: bytes at final offsets
__global__ __launch_bounds__(256) void ibwt_walk2_kernel(const u32 *__restrict__ spos, u32 N, u32 K,
                                                         const u32 *__restrict__ nxt,
                                                         const u32 *__restrict__ dist,
                                                         const u64 *__restrict__ scalars,
                                                         CTable ct, u8 *__restrict__ text,
                                                         const u32 *__restrict__ ovlist, u32 nov, u32 *err) {
    __shared__ u32 s_c[260];
    __shared__ i16 s_sym[260];
    ibwt_stage_ctable(ct, s_c, s_sym);
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nov) return;
    const u32 q = ovlist[i];            // a segment that did not fit its record buffer
    if (q >= K || !ibwt_on_chain(q, nxt)) return;
    u32 Lc, p = ibwt_chain_offset(q, dist, scalars, Lc);
    u32 r = ibwt_split_row(q), steps = 0;
    while (steps++ <= N) {
        r = spos[r];
        if (r == 0) break;
        int sym = ibwt_sym_of_row(s_c, s_sym, ct.sigma, r);
        if (sym < 0) {
            atomicOr(err, 0x200u);  // fromJust Nothing (BWT/Internal.hs:195)
            break;
        }
        text[p++] = (u8)sym;
        if (ibwt_is_splitter(r)) break;
    }
}

// every splitter on row e's chain copies its recorded segment to its final offset (one wave per
// splitter, 64 bytes per step)
__global__ __launch_bounds__(256) void ibwt_copy_kernel(u32 K, const u32 *__restrict__ nxt,
                                                        const u32 *__restrict__ dist,
                                                        const u64 *__restrict__ scalars,
                                                        const u8 *__restrict__ seg,
                                                        const u32 *__restrict__ seglen,
                                                        const u8 *__restrict__ segflag,
                                                        u8 *__restrict__ text, u32 *err) {
    const u32 q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= K) return;
    if (!ibwt_on_chain(q, nxt)) return;
    const u32 fl = segflag[q];
    if (fl & 2u) {
        if (lane_id() == 0) atomicOr(err, 0x200u);  // fromJust Nothing (BWT/Internal.hs:195)
        return;
    }
    if (fl & 1u) return;                // too long for its buffer: ibwt_walk2_kernel
    u32 Lc;
    const u32 p0 = ibwt_chain_offset(q, dist, scalars, Lc);
    const u32 len = seglen[q];
    const u8 *src = seg + (u64)q * IBWT_SEGCAP;
    for (u32 i = lane_id(); i < len; i += 64) text[p0 + i] = src[i];
}

// ---- small alphabets (<= 5 byte values, one Nothing): the walk by LF instead of by positions ------
// The position array of the sort above is 4 N bytes and every step of a walk reads 4 of them at a
// random place.  For DNA-like records the same step can be computed from the last column itself:
// LF(r) = C[c] + (occurrences of c = L[r] above row r) is the inverse of the step the reference
// takes (sorted[f].position), so walking it from row e = 0 visits the same cycle backwards and
// emits the text reversed.  The last column is kept as 64-byte lines of 128 rows: {occurrences of
// codes 0..3 above the line, three bit planes of the 3-bit codes}; a step reads ONE line of a
// structure of N / 2 bytes (0.5 GB for a 1 GiB record, half of it inside the 256 MB MALL) and
// needs no sort of the positions at all.  The Nothing row p is stored as code 0 and taken back out
// of code 0's counts; LF(p) = 0 closes the cycle.  Code 4's count is what is left of the line start.
#define LF_ROWS 128                 // rows per line
#define LF_BLOCK (256 * LF_ROWS)    // rows per block of the build kernels
#define LF_STRIDE 132               // staged bytes per line in LDS (33 words: conflict-free)
struct LfTable {
    u32 C[8];     // first sorted row of code c
    u8 sym[8];    // byte value of code c
};

// the symbols as MTF codes, one byte each (fused decode of a small alphabet): code 0 = Nothing,
// code c = the (c-1)-th byte value; as an accessor it yields c - 1, i.e. -1 or the LF code itself
struct CodeAcc {
    const u8 *c;
    __device__ __forceinline__ int operator()(u64 j) const { return (int)c[j] - 1; }
};
// pass 1: per block, occurrences of codes 0..3; the row of the Nothing -> *prim
// prim[0] = row of the (first) Nothing, prim[1] = number of Nothings, prim[2] != 0: a symbol outside the
// expected alphabet (lut value 0xff) was met
template <class Acc>
__global__ __launch_bounds__(256) void lf_count_kernel(Acc acc, u32 N, Lut8 lut, u32 *__restrict__ bcnt,
                                                       u32 *__restrict__ prim) {
    __shared__ u8 s_lut[260];
    __shared__ u32 s_c[4];
    for (int i = threadIdx.x; i < 257; i += 256) s_lut[i] = lut.v[i];
    if (threadIdx.x < 4) s_c[threadIdx.x] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * LF_BLOCK;
    u32 c[4] = {0, 0, 0, 0};
    auto one = [&](u64 j, int sym) {
        if (sym < 0) {
            atomicMin(prim, (u32)j);
            atomicAdd(prim + 1, 1u);
        }
        const u32 code = s_lut[sym + 1];
        if (code == 0xffu && !prim[2]) atomicOr(prim + 2, 1u);
        c[0] += code == 0; c[1] += code == 1; c[2] += code == 2; c[3] += code == 3;
    };
    bool done = false;
    if constexpr (std::is_same<Acc, SymAcc>::value) {
        // eight symbols per 16-byte load (2-byte loads run at a fraction of the HBM rate)
        if (base + LF_BLOCK <= N && (((uintptr_t)(acc.s + base)) & 15) == 0) {
            const uint4 *src = reinterpret_cast<const uint4 *>(acc.s + base);
            for (u32 g = threadIdx.x; g < LF_BLOCK / 8; g += 256) {
                const uint4 t = src[g];
                const u32 x[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int q = 0; q < 8; q++) one(base + 8 * g + q, (int)(i16)((x[q >> 1] >> (16 * (q & 1))) & 0xffffu));
            }
            done = true;
        }
    }
    if constexpr (std::is_same<Acc, CodeAcc>::value) {
        if (base + LF_BLOCK <= N && (((uintptr_t)(acc.c + base)) & 15) == 0) {
            const uint4 *src = reinterpret_cast<const uint4 *>(acc.c + base);
            for (u32 g = threadIdx.x; g < LF_BLOCK / 16; g += 256) {
                const uint4 t = src[g];
                const u32 x[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int q = 0; q < 16; q++) one(base + 16 * g + q, (int)((x[q >> 2] >> (8 * (q & 3))) & 0xffu) - 1);
            }
            done = true;
        }
    }
    if (!done)
        for (u32 i = threadIdx.x; i < LF_BLOCK; i += 256) {
            const u64 j = base + i;
            if (j >= N) break;
            one(j, acc(j));
        }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u32 v = c[k];
        for (int d = 32; d >= 1; d >>= 1) v += (u32)__shfl_xor((int)v, d, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&s_c[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 4) bcnt[(u64)blockIdx.x * 4 + threadIdx.x] = s_c[threadIdx.x];
}
// exclusive scan of the block counts, four counters side by side (one block)
__global__ __launch_bounds__(1024) void lf_scan_kernel(u32 *bcnt, u32 nb, u32 *__restrict__ totals) {
    __shared__ u32 s_part[1024][4];
    const u32 per = (nb + 1023) / 1024;
    const u32 lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    u32 v[4] = {0, 0, 0, 0};
    for (u32 t = lo; t < hi; t++)
        for (int k = 0; k < 4; k++) v[k] += bcnt[(u64)t * 4 + k];
    for (int k = 0; k < 4; k++) s_part[threadIdx.x][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        u32 run = 0;
        for (int i = 0; i < 1024; i++) {
            const u32 c = s_part[i][threadIdx.x];
            s_part[i][threadIdx.x] = run;
            run += c;
        }
        totals[threadIdx.x] = run;   // occurrences of codes 0..3 in the whole column
    }
    __syncthreads();
    u32 run[4];
    for (int k = 0; k < 4; k++) run[k] = s_part[threadIdx.x][k];
    for (u32 t = lo; t < hi; t++)
        for (int k = 0; k < 4; k++) {
            const u32 c = bcnt[(u64)t * 4 + k];
            bcnt[(u64)t * 4 + k] = run[k];
            run[k] += c;
        }
}
// pass 2: the lines
template <class Acc>
__global__ __launch_bounds__(256) void lf_build_kernel(Acc acc, u32 N, Lut8 lut, const u32 *__restrict__ bcnt,
                                                       uint4 *__restrict__ lines) {
    __shared__ u8 s_lut[260];
    __shared__ u32 s_code[256 * LF_STRIDE / 4];
    __shared__ u64 s_wsum[4];
    for (int i = threadIdx.x; i < 257; i += 256) s_lut[i] = lut.v[i];
    __syncthreads();
    const u64 base = (u64)blockIdx.x * LF_BLOCK;
    u8 *sc = reinterpret_cast<u8 *>(s_code);
    bool staged = false;
    if constexpr (std::is_same<Acc, SymAcc>::value) {
        if (base + LF_BLOCK <= N && (((uintptr_t)(acc.s + base)) & 15) == 0) {
            const uint4 *src = reinterpret_cast<const uint4 *>(acc.s + base);
            for (u32 g = threadIdx.x; g < LF_BLOCK / 8; g += 256) {
                const uint4 t = src[g];
                const u32 x[4] = {t.x, t.y, t.z, t.w};
                u32 w2[2] = {0, 0};
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const int sym = (int)(i16)((x[q >> 1] >> (16 * (q & 1))) & 0xffffu);
                    w2[q >> 2] |= (u32)s_lut[sym + 1] << (8 * (q & 3));
                }
                const u32 i = 8 * g;   // eight codes of one line: two aligned words
                u32 *dst = reinterpret_cast<u32 *>(sc + (i / LF_ROWS) * LF_STRIDE + (i % LF_ROWS));
                dst[0] = w2[0];
                dst[1] = w2[1];
            }
            staged = true;
        }
    }
    if constexpr (std::is_same<Acc, CodeAcc>::value) {
        if (base + LF_BLOCK <= N && (((uintptr_t)(acc.c + base)) & 15) == 0) {
            const uint4 *src = reinterpret_cast<const uint4 *>(acc.c + base);
            for (u32 g = threadIdx.x; g < LF_BLOCK / 16; g += 256) {
                const uint4 t = src[g];
                const u32 x[4] = {t.x, t.y, t.z, t.w};
                u32 w4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    w4[q] = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        w4[q] |= (u32)s_lut[(x[q] >> (8 * b)) & 0xffu] << (8 * b);   // lut index = (code - 1) + 1
                }
                const u32 i = 16 * g;   // sixteen codes of one line: four aligned words
                u32 *dst = reinterpret_cast<u32 *>(sc + (i / LF_ROWS) * LF_STRIDE + (i % LF_ROWS));
                dst[0] = w4[0]; dst[1] = w4[1]; dst[2] = w4[2]; dst[3] = w4[3];
            }
            staged = true;
        }
    }
    if (!staged)
        for (u32 i = threadIdx.x; i < LF_BLOCK; i += 256) {
            const u64 j = base + i;
            sc[(i / LF_ROWS) * LF_STRIDE + (i % LF_ROWS)] = j < N ? s_lut[acc(j) + 1] : (u8)0;
        }
    __syncthreads();
    const u32 *mine = s_code + threadIdx.x * (LF_STRIDE / 4);
    u64 pl[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
    for (int h = 0; h < 2; h++)
        for (int q = 0; q < 16; q++) {
            const u32 w = mine[h * 16 + q];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const u32 code = (w >> (8 * b)) & 7u;
                const int bit = q * 4 + b;
                pl[0][h] |= (u64)(code & 1u) << bit;
                pl[1][h] |= (u64)((code >> 1) & 1u) << bit;
                pl[2][h] |= (u64)((code >> 2) & 1u) << bit;
            }
        }
    // occurrences of codes 0..3 in this line, 16 bits each (a block holds 32768 rows)
    u64 cnt = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        u32 k = 0;
#pragma unroll
        for (int h = 0; h < 2; h++)
            k += (u32)__popcll(((c & 1) ? pl[0][h] : ~pl[0][h]) & ((c & 2) ? pl[1][h] : ~pl[1][h]) & ~pl[2][h]);
        cnt |= (u64)k << (16 * c);
    }
    // rows past N were staged as code 0: take them back out (only the last line of the text)
    {
        const u64 lstart = base + (u64)threadIdx.x * LF_ROWS;
        if (lstart + LF_ROWS > N) cnt -= (lstart >= N ? (u64)LF_ROWS : lstart + LF_ROWS - N);
    }
    u64 inc = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(inc, d, 64);
        if ((int)(threadIdx.x & 63) >= d) inc += t;
    }
    if ((threadIdx.x & 63) == 63) s_wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    u64 pre = inc - cnt;
    for (int i = 0; i < (int)(threadIdx.x >> 6); i++) pre += s_wsum[i];
    const u64 lstart = base + (u64)threadIdx.x * LF_ROWS;
    if (lstart < N) {
        const u32 *bc = bcnt + (u64)blockIdx.x * 4;
        uint4 *o = lines + (lstart / LF_ROWS) * 4;
        o[0] = make_uint4(bc[0] + (u32)(pre & 0xffff), bc[1] + (u32)((pre >> 16) & 0xffff),
                          bc[2] + (u32)((pre >> 32) & 0xffff), bc[3] + (u32)(pre >> 48));
        o[1] = make_uint4((u32)pl[0][0], (u32)(pl[0][0] >> 32), (u32)pl[0][1], (u32)(pl[0][1] >> 32));
        o[2] = make_uint4((u32)pl[1][0], (u32)(pl[1][0] >> 32), (u32)pl[1][1], (u32)(pl[1][1] >> 32));
        o[3] = make_uint4((u32)pl[2][0], (u32)(pl[2][0] >> 32), (u32)pl[2][1], (u32)(pl[2][1] >> 32));
    }
}

// one LF step; `code` = the code of L[r].  r == p (the Nothing row): LF = 0
__device__ __forceinline__ u32 lf_step(const uint4 *__restrict__ lines, const u32 *s_C, u32 p, u32 r, u32 &code) {
    const uint4 *ln = lines + (u64)(r / LF_ROWS) * 4;
    const uint4 a = ln[0], b0 = ln[1], b1 = ln[2], b2 = ln[3];
    const u32 o = r % LF_ROWS, hi = o >> 6, sh = o & 63u;
    const u64 p0[2] = {(u64)b0.x | ((u64)b0.y << 32), (u64)b0.z | ((u64)b0.w << 32)};
    const u64 p1[2] = {(u64)b1.x | ((u64)b1.y << 32), (u64)b1.z | ((u64)b1.w << 32)};
    const u64 p2[2] = {(u64)b2.x | ((u64)b2.y << 32), (u64)b2.z | ((u64)b2.w << 32)};
    const u32 c0 = (u32)((hi ? p0[1] : p0[0]) >> sh) & 1u, c1 = (u32)((hi ? p1[1] : p1[0]) >> sh) & 1u,
              c2 = (u32)((hi ? p2[1] : p2[0]) >> sh) & 1u;
    code = c0 | (c1 << 1) | (c2 << 2);
    const u64 m0 = (c0 ? p0[0] : ~p0[0]) & (c1 ? p1[0] : ~p1[0]) & (c2 ? p2[0] : ~p2[0]);
    const u64 m1 = (c0 ? p0[1] : ~p0[1]) & (c1 ? p1[1] : ~p1[1]) & (c2 ? p2[1] : ~p2[1]);
    const u64 below = (1ull << sh) - 1ull;
    const u32 in_line = hi ? (u32)__popcll(m0) + (u32)__popcll(m1 & below) : (u32)__popcll(m0 & below);
    const u32 lstart = r - o;
    const u32 above = code == 0 ? a.x : code == 1 ? a.y : code == 2 ? a.z : code == 3 ? a.w
                                                                              : lstart - (a.x + a.y + a.z + a.w);
    if (r == p) return 0u;
    return s_C[code] + above + in_line - ((code == 0 && r > p) ? 1u : 0u);
}

// the walks of ibwt_walk1_kernel with the LF step (same records, same chain bookkeeping)
__global__ __launch_bounds__(256) void ibwt_lfwalk1_kernel(const uint4 *__restrict__ lines, u32 N, u32 K,
                                                           const u32 *__restrict__ prim, LfTable tb,
                                                           u32 *__restrict__ nxt, u32 *__restrict__ dist,
                                                           u8 *__restrict__ seg, u32 *__restrict__ seglen,
                                                           u8 *__restrict__ segflag, u32 force_rewalk,
                                                           u32 *__restrict__ noverflow, u32 *__restrict__ ovlist,
                                                           u32 *__restrict__ nextra, u32 extra_cap, u32 segcap) {
    __shared__ u32 s_C[8];
    __shared__ u8 s_sym[8];
    if (threadIdx.x < 8) {
        s_C[threadIdx.x] = tb.C[threadIdx.x];
        s_sym[threadIdx.x] = tb.sym[threadIdx.x];
    }
    __syncthreads();
    const u32 p = *prim;
    const u32 q = blockIdx.x * 256 + threadIdx.x;
    if (q >= K) return;
    u32 r = ibwt_split_row(q);
    if (r >= N) {
        ibwt_inert_slot(q, nxt, dist, seglen, segflag);
        return;
    }
    SegRecorder rec{seg, nxt, dist, seglen, segflag};
    rec.open(q, force_rewalk ? 1u : 0u);
    for (;;) {
        rec.steps++;
        u32 code;
        const u32 rn = lf_step(lines, s_C, p, r, code);
        if (rn != 0) rec.put((u32)s_sym[code]);   // (rn == 0: r was the Nothing row -- nothing to emit)
        r = rn;
        if (ibwt_is_splitter(r) || rec.steps > N) break;
        rec.extend_if_full(K, segcap, nextra, extra_cap);
    }
    rec.close(r / IBWT_S);
    if (rec.flag & 1u) ovlist[atomicAdd(noverflow, 1u)] = rec.q;
}
// segments that did not fit their record buffer: walked again, bytes at their final (reversed) offsets
__global__ __launch_bounds__(256) void ibwt_lfwalk2_kernel(const uint4 *__restrict__ lines, u32 N, u32 K,
                                                           const u32 *__restrict__ prim, LfTable tb,
                                                           const u32 *__restrict__ nxt, const u32 *__restrict__ dist,
                                                           const u64 *__restrict__ scalars, u8 *__restrict__ text,
                                                           const u32 *__restrict__ ovlist, u32 nov) {
    __shared__ u32 s_C[8];
    __shared__ u8 s_sym[8];
    if (threadIdx.x < 8) {
        s_C[threadIdx.x] = tb.C[threadIdx.x];
        s_sym[threadIdx.x] = tb.sym[threadIdx.x];
    }
    __syncthreads();
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nov) return;
    const u32 q = ovlist[i];
    if (q >= K || !ibwt_on_chain(q, nxt)) return;
    const u32 p = *prim;
    u32 Lc, k = ibwt_chain_offset(q, dist, scalars, Lc);   // offset in the reversed text
    u32 r = ibwt_split_row(q), steps = 0;
    while (steps++ <= N) {
        u32 code;
        r = lf_step(lines, s_C, p, r, code);
        if (r == 0) break;
        if (k + 2 <= Lc) text[Lc - 2 - k] = s_sym[code];
        k++;
        if (ibwt_is_splitter(r)) break;
    }
}
// ibwt_copy_kernel for the reversed walk.  A wave per splitter: the record comes in with 16-byte
// loads (into LDS), leaves mirrored with 4-byte stores (one-byte copies ran at 1.2 TB/s).
__global__ __launch_bounds__(256) void ibwt_copy_rev_kernel(u32 K, const u32 *__restrict__ nxt,
                                                            const u32 *__restrict__ dist,
                                                            const u64 *__restrict__ scalars,
                                                            const u8 *__restrict__ seg,
                                                            const u32 *__restrict__ seglen,
                                                            const u8 *__restrict__ segflag,
                                                            u8 *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) u8 s_seg[4][IBWT_SEGCAP];
    const u32 w = threadIdx.x >> 6, l = lane_id();
    const u32 q = blockIdx.x * 4 + w;
    if (q >= K) return;
    if (!ibwt_on_chain(q, nxt)) return;
    if (segflag[q] & 1u) return;
    u32 Lc;
    const u32 k0 = ibwt_chain_offset(q, dist, scalars, Lc);
    u32 len = seglen[q];
    if (k0 + 2 > Lc) return;
    if (len > Lc - 1 - k0) len = Lc - 1 - k0;       // (a valid chain never needs this)
    if (len == 0) return;
    const u8 *src = seg + (u64)q * IBWT_SEGCAP;
    u8 *sb = s_seg[w];
    for (u32 i = l * 16; i < len; i += 64 * 16)
        *reinterpret_cast<uint4 *>(sb + i) = *reinterpret_cast<const uint4 *>(src + i);
    __builtin_amdgcn_wave_barrier();
    // text[D - i] = src[i]; the destination bytes are [D - len + 1, D]
    const u64 D = (u64)Lc - 2 - k0;
    u8 *lo = text + (D - len + 1), *hi = text + D + 1;                 // [lo, hi)
    u8 *alo = reinterpret_cast<u8 *>((reinterpret_cast<uintptr_t>(lo) + 3) & ~(uintptr_t)3);
    u8 *ahi = reinterpret_cast<u8 *>(reinterpret_cast<uintptr_t>(hi) & ~(uintptr_t)3);
    if (alo >= ahi) {   // shorter than an aligned word: bytes
        for (u32 i = l; i < len; i += 64) text[D - i] = sb[i];
        return;
    }
    const u32 head = (u32)(alo - lo), tail = (u32)(hi - ahi), words = (u32)(ahi - alo) / 4;
    if (l < head) lo[l] = sb[len - 1 - l];
    if (l < tail) ahi[l] = sb[(u32)(hi - ahi) - 1 - l];
    for (u32 j = l; j < words; j += 64) {
        const u32 i3 = (u32)(text + D - (alo + 4 * j));   // source index of the word's first byte
        const u32 v = (u32)sb[i3] | ((u32)sb[i3 - 1] << 8) | ((u32)sb[i3 - 2] << 16) | ((u32)sb[i3 - 3] << 24);
        *reinterpret_cast<u32 *>(alo + 4 * j) = v;
    }
}

#endif  // __HIPCC__
