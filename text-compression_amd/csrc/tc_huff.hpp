// tc_huff.hpp -- the entropy-coded body of a container (format 3): canonical, length-limited Huffman coding of a
// tc_block's runs.  An addition to the reference's surface, as the container itself is (the reference has no wire
// format); the layout is written down in include/textcomp.h and restated in tests/huffman_format.py.
//
// Tokens: sigma + 2 symbols.  A run (value v, count c >= 1) is the token v followed by the floor(log2 c) low bits of c,
// least significant first, one token per bit: RUNA = sigma for a 0 bit, RUNB = sigma + 1 for a 1 bit -- the digits of
// c - 1 in bijective base 2 (bzip2's run digits, applied to every value).  So the digit tokens of a run are counted
// in closed form: RUNB = popcount(c) - 1, RUNA = floor(log2 c) - RUNB.
//
// Writer: huff_hist_kernel (token histogram + what the fixed-width packing would cost, one pass over the runs), code
// lengths on the host (package-merge over <= 259 weights), huff_encode_kernel<false> (bits per chunk of HF_K runs),
// huff_dir_scan_kernel (chunk starts), huff_encode_kernel<true> (the bits: assembled in LDS by 32-bit atomicOr, written
// as whole words; every chunk starts at a word of its own, so no two workgroups ever touch the same word).
// Reader: huff_dir_scan_kernel, then huff_decode_kernel (a lane walks a chunk with one table lookup per token).
#pragma once
#include <algorithm>
#include <utility>

#include "tc_common.hpp"
#include "tc_pack.hpp"

#define HF_FORMAT 3
#define HF_LMAX 12                       // longest code: one decode table of 2^12 two-byte entries (8 KB of LDS)
#define HF_K 1024                        // runs per chunk (what the writer uses; a reader takes any power of two)
#define HF_MAXSYM (TC_MAX_SIGMA + 2)     // 259 tokens at most
#define HF_NT 256
#define HF_RPT (HF_K / HF_NT)            // consecutive runs of a chunk per thread
#define HF_IMG_WORDS 1024                // LDS window a chunk's bits are assembled in (longer chunks: several windows)
#define HF_ERR_FLAG 0x800u               // device error word: malformed Huffman body (tc_sync_check: TC_ERR_MALFORMED)
#define HF_TOT_WORDS 16                  // u32 words behind the histogram that hold the u64 totals below
#define HF_HIST_WORDS (264 + HF_TOT_WORDS)
static_assert(HF_K % HF_NT == 0 && (HF_K & (HF_K - 1)) == 0, "a chunk is a power of two of runs, split evenly over the workgroup");
static_assert((1u << HF_LMAX) >= HF_MAXSYM, "every token can have a code");
static_assert((HF_NT / 64) * (HF_MAXSYM + 1) * 4 + 64 <= 16 * 1024, "histogram kernel: LDS budget");
static_assert(HF_IMG_WORDS * 4 + HF_MAXSYM * 4 + 64 <= 16 * 1024, "encode kernel: LDS budget");
static_assert((2u << HF_LMAX) + 2 * HF_MAXSYM + 128 <= 16 * 1024, "decode kernel: LDS budget");

static inline u64 hf_pad16(u64 b) { return (b + 15) & ~15ull; }
// bytes of head + lengths + directory (each padded to 16)
static inline u64 hf_fixed_bytes(u32 nsyms, u64 nchunks) { return 16 + hf_pad16(nsyms) + hf_pad16(4 * nchunks); }

// ---- 1: token histogram and the size of the fixed-width packing, one pass ------------------------------------------
struct HuffHistArgs {
    const u32 *cnt;
    const u16 *val;
    u64 nruns;
    u32 sigma;
    u32 *hist;   // [HF_HIST_WORDS], ZERO: token counts [0, sigma + 2); then, as u64 at hist + 264:
                 // [0] nibbles of the nibble stream, [1] counts outside 1..4, [2] counts >= 15, [3] counts >= 127,
                 // [4] runs the token scheme has no code for (count 0, value >= sigma)
};

__global__ __launch_bounds__(HF_NT) void huff_hist_kernel(HuffHistArgs a) {
    constexpr int NW = HF_NT / 64;
    __shared__ u32 s_h[NW][HF_MAXSYM + 1];
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    for (int i = tid; i < NW * (HF_MAXSYM + 1); i += HF_NT) (&s_h[0][0])[i] = 0;
    __syncthreads();
    // the hot bins stay in registers (most tokens of a BWT record are value 0 and the run digits): the LDS atomics
    // see the values from 4 on only
    u32 h0 = 0, h1 = 0, h2 = 0, h3 = 0, ra = 0, rb = 0;
    u32 nib = 0, e4 = 0, e15 = 0, e127 = 0, bad = 0;
    const u32 sigma = a.sigma;
    for (u64 i = (u64)blockIdx.x * HF_NT + tid; i < a.nruns; i += (u64)gridDim.x * HF_NT) {
        const u32 c = a.cnt[i], v = a.val[i];
        if (c == 0 || v >= sigma) {
            bad++;
        } else {
            const u32 nd = 31u - (u32)__builtin_clz(c), nb = (u32)__popc(c) - 1u;
            ra += nd - nb;
            rb += nb;
            h0 += v == 0; h1 += v == 1; h2 += v == 2; h3 += v == 3;
            if (v >= 4) atomicAdd(&s_h[w][v], 1u);
        }
        const u32 c1 = c - 1u;
        nib += c1 < 2u ? 1u : 2u;
        e4 += c1 >= 4u;
        e15 += c >= 15u;
        e127 += c >= 127u;
    }
    h0 = wave_sum(h0); h1 = wave_sum(h1); h2 = wave_sum(h2); h3 = wave_sum(h3);
    ra = wave_sum(ra); rb = wave_sum(rb);
    nib = wave_sum(nib); e4 = wave_sum(e4); e15 = wave_sum(e15); e127 = wave_sum(e127); bad = wave_sum(bad);
    if (lane == 0) {
        // (sigma >= 1 here; bins 0..3 of an alphabet smaller than 4 stay 0 because v < sigma)
        s_h[w][0] += h0; s_h[w][1] += h1; s_h[w][2] += h2; s_h[w][3] += h3;
        s_h[w][sigma] += ra; s_h[w][sigma + 1] += rb;
        unsigned long long *tot = reinterpret_cast<unsigned long long *>(a.hist + 264);
        if (nib) atomicAdd(tot + 0, (unsigned long long)nib);
        if (e4) atomicAdd(tot + 1, (unsigned long long)e4);
        if (e15) atomicAdd(tot + 2, (unsigned long long)e15);
        if (e127) atomicAdd(tot + 3, (unsigned long long)e127);
        if (bad) atomicAdd(tot + 4, (unsigned long long)bad);
    }
    __syncthreads();
    for (u32 b = tid; b < sigma + 2u; b += HF_NT) {
        u32 t = 0;
#pragma unroll
        for (int i = 0; i < NW; i++) t += s_h[i][b];
        if (t) atomicAdd(&a.hist[b], t);
    }
}

// ---- 2: code lengths (host) ------------------------------------------------------------------------------------------
// Package-merge: the optimal code under the length limit.  Deterministic: symbols in (weight, index) order, a
// package goes behind a symbol of equal weight.  A token that does not occur gets length 0 (no code); a record with a
// single distinct token gets length 1.
static inline void huff_build_lengths(const u32 *hist, u32 nsyms, u8 *len) {
    std::vector<u32> syms;
    for (u32 s = 0; s < nsyms; s++) {
        len[s] = 0;
        if (hist[s]) syms.push_back(s);
    }
    const size_t m = syms.size();
    if (m == 0) return;
    if (m == 1) { len[syms[0]] = 1; return; }
    std::stable_sort(syms.begin(), syms.end(), [&](u32 x, u32 y) { return hist[x] < hist[y]; });
    struct Item { u64 w; std::vector<u16> cover; };   // cover[j]: how often leaf j (sorted order) lies in this item
    std::vector<Item> leaves(m), prev, cur;
    for (size_t j = 0; j < m; j++) {
        leaves[j].w = hist[syms[j]];
        leaves[j].cover.assign(m, 0);
        leaves[j].cover[j] = 1;
    }
    prev = leaves;
    for (int level = 1; level < HF_LMAX; level++) {
        std::vector<Item> pk;
        for (size_t i = 0; i + 1 < prev.size(); i += 2) {
            Item p;
            p.w = prev[i].w + prev[i + 1].w;
            p.cover = prev[i].cover;
            for (size_t j = 0; j < m; j++) p.cover[j] += prev[i + 1].cover[j];
            pk.push_back(std::move(p));
        }
        cur.clear();
        size_t x = 0, y = 0;
        while (x < m || y < pk.size()) {
            if (y >= pk.size() || (x < m && leaves[x].w <= pk[y].w)) cur.push_back(leaves[x++]);
            else cur.push_back(std::move(pk[y++]));
        }
        prev.swap(cur);
    }
    for (size_t i = 0; i < 2 * m - 2; i++)
        for (size_t j = 0; j < m; j++) len[syms[j]] += (u8)prev[i].cover[j];
}

// canonical codes from lengths: (length, symbol) order starting from 0; code[s] = bits | length << 16
struct HuffCodes {
    u32 v[HF_MAXSYM + 1];
};
static inline void huff_assign_codes(const u8 *len, u32 nsyms, HuffCodes *out) {
    u32 next[HF_LMAX + 2] = {0}, count[HF_LMAX + 2] = {0};
    for (u32 s = 0; s < nsyms; s++) count[len[s]]++;
    count[0] = 0;
    u32 code = 0;
    for (int l = 1; l <= HF_LMAX; l++) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    memset(out, 0, sizeof *out);
    for (u32 s = 0; s < nsyms; s++)
        if (len[s]) out->v[s] = next[len[s]]++ | ((u32)len[s] << 16);
}

// ---- 3: the bits --------------------------------------------------------------------------------------------------------
struct HuffEncArgs {
    const u32 *cnt;
    const u16 *val;
    u64 nruns;
    u32 sigma;
    u32 nchunks;
    u32 *dirbits;        // [nchunks] bits of every chunk (WRITE = false: out; true: in)
    const u64 *offs;     // [nchunks + 1] first payload word of every chunk (WRITE only)
    u32 *payload;        // (WRITE only)
    u64 payload_words;   // capacity of `payload`
    HuffCodes codes;
};

// bits of one run; a run without a code (the histogram pass has refused the record then) counts as nothing
__device__ __forceinline__ u32 hf_run_bits(const u32 *tab, u32 sigma, u32 c, u32 v) {
    if (c == 0 || v >= sigma) return 0;
    const u32 nd = 31u - (u32)__builtin_clz(c), nb = (u32)__popc(c) - 1u;
    return (tab[v] >> 16) + (nd - nb) * (tab[sigma] >> 16) + nb * (tab[sigma + 1] >> 16);
}

// the `n` low bits of `acc` (first bit of the string = the highest of them) go to bit position `pos` of the chunk's
// stream, of which the LDS image holds the words [w0, w0 + HF_IMG_WORDS); stream bit b is bit 31 - (b & 31) of word b >> 5
__device__ __forceinline__ void hf_flush(u32 *img, u32 w0, u32 pos, u64 acc, u32 n) {
    u32 wd = pos >> 5, o = pos & 31u;
    while (n) {
        const u32 room = 32u - o, take = n < room ? n : room;
        const u32 piece = (u32)((acc >> (n - take)) & ((1ull << take) - 1ull));
        const u32 wi = wd - w0;
        if (wi < HF_IMG_WORDS && piece) atomicOr(&img[wi], piece << (room - take));
        n -= take;
        o = 0;
        wd++;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(HF_NT) void huff_encode_kernel(HuffEncArgs a) {
    __shared__ u32 s_tab[HF_MAXSYM + 1];
    __shared__ u32 s_scan[HF_NT / 64 + 1];
    __shared__ u32 s_img[WRITE ? HF_IMG_WORDS : 1];
    const int tid = threadIdx.x;
    for (int i = tid; i < HF_MAXSYM + 1; i += HF_NT) s_tab[i] = a.codes.v[i];
    __syncthreads();
    const u32 sigma = a.sigma;
    const u32 ea = s_tab[sigma], eb = s_tab[sigma + 1];
    for (u32 k = blockIdx.x; k < a.nchunks; k += gridDim.x) {
        const u64 r0 = (u64)k * HF_K + (u64)tid * HF_RPT;
        u32 c[HF_RPT], v[HF_RPT], bits = 0;
#pragma unroll
        for (int j = 0; j < HF_RPT; j++) {
            const bool ok = r0 + j < a.nruns;
            c[j] = ok ? a.cnt[r0 + j] : 0u;
            v[j] = ok ? a.val[r0 + j] : 0u;
            bits += hf_run_bits(s_tab, sigma, c[j], v[j]);
        }
        u32 total;
        const u32 start = block_excl_sum<HF_NT>(bits, s_scan, &total);
        if (!WRITE) {
            if (tid == 0) a.dirbits[k] = total;
            __syncthreads();   // s_scan is read by everybody before the next chunk overwrites it
            continue;
        }
        const u32 nwords = (total + 31u) >> 5;
        const u64 off = a.offs[k];
        for (u32 w0 = 0; w0 < nwords; w0 += HF_IMG_WORDS) {
            const u32 nw = nwords - w0 < HF_IMG_WORDS ? nwords - w0 : HF_IMG_WORDS;
            __syncthreads();   // the previous image has left
            for (u32 i = tid; i < nw; i += HF_NT) s_img[i] = 0;
            __syncthreads();
            // this thread's bits lie in [start, start + bits): skip the walk when they miss the window
            if (bits && (start >> 5) < w0 + nw && ((start + bits - 1u) >> 5) >= w0) {
                u32 pos = start, n = 0;
                u64 acc = 0;
                auto put = [&](u32 e) {   // e = bits | length << 16
                    const u32 l = e >> 16;
                    if (n + l > 64u) {
                        hf_flush(s_img, w0, pos, acc, n);
                        pos += n; n = 0; acc = 0;
                    }
                    acc = (acc << l) | (u64)(e & 0xffffu);
                    n += l;
                };
#pragma unroll
                for (int j = 0; j < HF_RPT; j++) {
                    if (c[j] == 0 || v[j] >= sigma) continue;
                    put(s_tab[v[j]]);
                    const u32 nd = 31u - (u32)__builtin_clz(c[j]);
                    for (u32 d = 0; d < nd; d++) put(((c[j] >> d) & 1u) ? eb : ea);   // (rarely more than a turn or two)
                }
                hf_flush(s_img, w0, pos, acc, n);
            }
            __syncthreads();
            for (u32 i = tid; i < nw; i += HF_NT)
                if (off + w0 + i < a.payload_words) a.payload[off + w0 + i] = s_img[i];
        }
        __syncthreads();
    }
}

// ---- chunk starts: exclusive prefix sum of the chunks' word counts, one workgroup -------------------------------------
// offs[k] = sum over j < k of ceil(dirbits[j] / 32); offs[nchunks] = payload words.  64-bit throughout: a reader runs
// this over a directory it has not validated yet.
#define HF_SCAN_NT 1024
#define HF_SCAN_PER 8
__global__ __launch_bounds__(HF_SCAN_NT) void huff_dir_scan_kernel(const u32 *__restrict__ dirbits, u64 nchunks, u64 *__restrict__ offs) {
    __shared__ u64 s_w[HF_SCAN_NT / 64];
    __shared__ u64 s_carry;
    const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < nchunks; base += (u64)HF_SCAN_NT * HF_SCAN_PER) {
        const u64 i0 = base + (u64)tid * HF_SCAN_PER;
        u64 x[HF_SCAN_PER], sum = 0;
#pragma unroll
        for (int j = 0; j < HF_SCAN_PER; j++) {
            x[j] = i0 + j < nchunks ? ((u64)dirbits[i0 + j] + 31ull) >> 5 : 0ull;
            sum += x[j];
        }
        u64 inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        u64 before = s_carry, tot = 0;
#pragma unroll
        for (int i = 0; i < HF_SCAN_NT / 64; i++) {
            const u64 t = s_w[i];
            if (i < w) before += t;
            tot += t;
        }
        u64 run = before + inc - sum;
#pragma unroll
        for (int j = 0; j < HF_SCAN_PER; j++) {
            if (i0 + j < nchunks) offs[i0 + j] = run;
            run += x[j];
        }
        __syncthreads();
        if (tid == 0) s_carry += tot;
        __syncthreads();
    }
    if (tid == 0) offs[nchunks] = s_carry;
}

// ---- 4: decode ----------------------------------------------------------------------------------------------------------
struct HuffDecArgs {
    const u8 *len;        // [nsyms] code lengths (validated by the host: <= lmax, Kraft sum <= 1)
    const u32 *dirbits;   // [nchunks]
    const u64 *offs;      // [nchunks + 1] (huff_dir_scan_kernel; offs[nchunks] == payload_words checked by the host)
    const u32 *payload;
    u64 payload_words;
    u64 nruns;            // <= the capacity of cnt / val (checked by the host)
    u32 K, nchunks, sigma, lmax;
    u32 *cnt;
    u16 *val;
    u32 *err;
};

// table entry: token | length << 9; HF_TAB_NONE: no code starts with these bits
#define HF_TAB_NONE 0xffffu
__global__ __launch_bounds__(HF_NT) void huff_decode_kernel(HuffDecArgs a) {
    __shared__ u16 s_tab[1u << HF_LMAX];
    __shared__ u8 s_len[HF_MAXSYM + 5];
    __shared__ u32 s_first[HF_LMAX + 2];
    const int tid = threadIdx.x;
    const u32 nsyms = a.sigma + 2u, lmax = a.lmax;   // (host: nsyms <= HF_MAXSYM, 1 <= lmax <= HF_LMAX)
    const u32 tsize = 1u << lmax;
    for (u32 i = tid; i < tsize; i += HF_NT) s_tab[i] = HF_TAB_NONE;
    for (u32 i = tid; i < nsyms; i += HF_NT) {
        const u32 l = a.len[i];
        s_len[i] = (u8)(l <= lmax ? l : 0u);
    }
    __syncthreads();
    if (tid == 0) {   // first code of every length
        u32 count[HF_LMAX + 2];
        for (u32 l = 0; l <= HF_LMAX + 1; l++) count[l] = 0;
        for (u32 s = 0; s < nsyms; s++) count[s_len[s]]++;
        count[0] = 0;
        u32 code = 0;
        s_first[0] = 0;
        for (u32 l = 1; l <= HF_LMAX; l++) {
            code = (code + count[l - 1]) << 1;
            s_first[l] = code;
        }
    }
    __syncthreads();
    for (u32 s = tid; s < nsyms; s += HF_NT) {
        const u32 l = s_len[s];
        if (l == 0) continue;
        u32 code = s_first[l];
        for (u32 t = 0; t < s; t++) code += s_len[t] == l;
        const u32 span = 1u << (lmax - l);
        const u64 lo = (u64)code << (lmax - l);
        for (u32 i = 0; i < span; i++)
            if (lo + i < tsize) s_tab[lo + i] = (u16)(s | (l << 9));   // (a Kraft sum <= 1 keeps every code inside the table)
    }
    __syncthreads();
    const u32 sigma = a.sigma;
    for (u64 k = (u64)blockIdx.x * HF_NT + tid; k < a.nchunks; k += (u64)gridDim.x * HF_NT) {
        const u64 r0 = k * a.K;
        const u64 want = a.nruns - r0 < a.K ? a.nruns - r0 : a.K;   // (host: nchunks = ceil(nruns / K), so r0 < nruns)
        const u32 nbits = a.dirbits[k];
        const u64 off = a.offs[k], nw = ((u64)nbits + 31ull) >> 5;
        bool bad = off + nw > a.payload_words;
        u64 buf = 0, wp = off, got = 0;
        const u64 wend = off + nw;
        u32 have = 0, pos = 0;
        bool open = false;
        u32 cv = 0, cb = 0, nd = 0;
        while (!bad && pos < nbits) {
            while (have <= 32u && wp < wend) {
                buf |= (u64)a.payload[wp++] << (32u - have);
                have += 32u;
            }
            const u32 e = s_tab[(u32)(buf >> (64u - lmax))];
            const u32 l = e >> 9, t = e & 511u;
            if (e == HF_TAB_NONE || pos + l > nbits) { bad = true; break; }   // no such code / the chunk ends inside a code
            buf <<= l; have -= l; pos += l;
            if (t < sigma) {
                if (open) {
                    a.cnt[r0 + got] = cb | (1u << nd);
                    a.val[r0 + got] = (u16)cv;
                    got++;
                }
                if (got >= want) { bad = true; break; }    // more runs than the chunk may hold
                open = true; cv = t; cb = 0; nd = 0;
            } else {
                if (!open || nd >= 31u) { bad = true; break; }   // a digit before any value / a count above 2^32 - 1
                cb |= (t - sigma) << nd;
                nd++;
            }
        }
        if (!bad && open) {
            a.cnt[r0 + got] = cb | (1u << nd);
            a.val[r0 + got] = (u16)cv;
            got++;
        }
        if (bad || got != want) atomicOr(a.err, HF_ERR_FLAG);
    }
}
