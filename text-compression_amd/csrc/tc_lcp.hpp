// tc_lcp.hpp -- the LCP array of a text from its suffix array, on the device.  No counterpart in
// the reference.  Included by tc_lcp_host.hpp; host/check/lcp_kernels.cpp compiles the same kernel bodies as plain C++
// (TC_LCP_HOST_CHECK: the HIP keywords defined away, a workgroup of one lane, the lanes of a grid run one after another).
//
// Rows and positions.  sa has N = n + 1 rows, row 0 the empty suffix (sa[0] = n).  lcp[0] = 0 and lcp[j] = the longest
// common prefix of the suffixes at sa[j - 1] and sa[j]; the end of the text matches nothing.  The work is done in TEXT
// order: phi[i] = the start of the suffix that precedes suffix i in the suffix array, PLCP[i] = lcp(i, phi[i]).  Position
// i is reducible when i > 0, phi[i] > 0 and T[i - 1] == T[phi[i] - 1]; then PLCP[i] = PLCP[i - 1] - 1.  So PLCP[i] + i
// never falls, and it equals the running maximum of V[k] = PLCP[k] + k over the IRREDUCIBLE positions k <= i: only those
// are compared byte by byte, and their values sum to at most 2 n log2 n for every text (Karkkainen, Manzini, Puglisi,
// CPM 2009).  Five steps, each one kernel (the scan three):
//   1  lcp_phi_kernel          phi[sa[j]] = sa[j - 1], j >= 1, over an array preset to LCP_UNSET
//   2  lcp_irreducible_kernel  one lane per position: reducible -> V = 0; else compare in 16-byte loads up to the short
//                              cap; a value that reaches the cap goes to the list of long items (phi[i] stays)
//   3  lcp_long_kernel         one workgroup per long item, 16 bytes per lane per load, two loads a side in flight; one wave's
//                              lanes load in the first turn, two waves' in the second, then all
//   4  lcp_scan_*_kernel       inclusive max-scan of V in place: tile maxima, their scan by one workgroup, the tiles
//   5  lcp_gather_kernel       lcp[j] = scan[sa[j]] - sa[j], saturating at 0 and clamped to n - max(sa[j - 1], sa[j])
// V overwrites phi in place: a lane (a workgroup in step 3) reads and writes its own slot only.
//
// What is read.  The text is n bytes and no kernel reads T[n] or beyond, or T[-1]: a 16-byte load at offset l of the pair
// (i, p) is issued only when l + 16 <= n - max(i, p), the bytes after that are read one at a time, and T[i - 1] only
// for i > 0.  The loads are unaligned (the two sides of a comparison differ by any distance), as 8-byte halves.
// A suffix array that is no permutation of 0 .. n raises LCP_ERR_SA (TC_ERR_MALFORMED) and stays in bounds: a row above
// n is never used as an index (steps 1 and 5 test it), so every phi entry is <= n or LCP_UNSET; a value that appears
// twice or is missing leaves a second slot unset, which step 2 finds (the one slot a permutation leaves unset is sa[0]);
// the list of long items is written below its capacity only.  A permutation that is not this text's suffix array gives
// values without meaning, which step 5 keeps within what the header promises.
#pragma once
#ifdef TC_LCP_HOST_CHECK
#include <stdint.h>
typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
#else
#include "tc_common.hpp"
#endif

#define TC_LCP_SHORT_CAP 256u    // step 2 stops here (a multiple of 16; tc_dbg_lcp_set_short_cap sets another per context: scripts/lcp_bench.py sweeps it)
#define LCP_UNSET 0xffffffffu    // phi of the one position without a predecessor (no position is that large: n <= TC_MAX_N)
#define LCP_ERR_SA 0x2000u       // device error bit: the suffix array is no permutation of 0 .. n (in 0xff00: TC_ERR_MALFORMED)
#define LCP_SCAN_ITEMS 16        // values per lane of a scan tile

#ifdef TC_LCP_HOST_CHECK
// ---- plain C++: one lane per workgroup; the launcher of host/check/lcp_kernels.cpp sets lcp_block / lcp_grid
#define LCP_NT 1
#define LCP_SCAN_NT 1
#define LCP_KERNEL static void
#define LCP_DEVICE static inline
#define LCP_SHARED static
static u32 lcp_block = 0, lcp_grid = 1;
static inline u32 lcp_tid() { return 0; }
static inline u32 lcp_bid() { return lcp_block; }
static inline u32 lcp_nblocks() { return lcp_grid; }
static inline void lcp_sync() {}
static inline void lcp_flag(u32 *err, u32 bits) { *err |= bits; }
static inline u32 lcp_ctz64(u64 x) { return (u32)__builtin_ctzll(x); }
static inline u32 lcp_load_u32(const u32 *p) { return *p; }
// a wave of one lane
static inline u32 lcp_wave_append(bool want, u32 *count) { return want ? (*count)++ : 0; }
template <int NT> static inline u32 lcp_block_min(u32 v, u32 *) { return v; }
template <int NT> static inline u32 lcp_block_excl_max(u32 v, u32 *, u32 *total) { *total = v; return 0; }
static inline void lcp_summary_publish(u64 key, u64 sum, u64 *, u64 *out2) {
    if (key > out2[0]) out2[0] = key;
    out2[1] += sum;
}
#else
#define LCP_NT 256
#define LCP_SCAN_NT 256
#define LCP_KERNEL __global__ void
#define LCP_DEVICE __device__ __forceinline__
#define LCP_SHARED __shared__
LCP_DEVICE u32 lcp_tid() { return threadIdx.x; }
LCP_DEVICE u32 lcp_bid() { return blockIdx.x; }
LCP_DEVICE u32 lcp_nblocks() { return gridDim.x; }
LCP_DEVICE void lcp_sync() { __syncthreads(); }
LCP_DEVICE void lcp_flag(u32 *err, u32 bits) { atomicOr(err, bits); }
LCP_DEVICE u32 lcp_ctz64(u64 x) { return (u32)__builtin_ctzll(x); }
LCP_DEVICE u32 lcp_load_u32(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one slot of a list per lane that wants one: one atomic per wave (a ballot counts the lanes, the first of them draws)
LCP_DEVICE u32 lcp_wave_append(bool want, u32 *count) {
    const u64 mask = __ballot(want);
    if (!mask) return 0;
    const int leader = __builtin_ctzll(mask);
    u32 base = 0;
    if ((int)lane_id() == leader) base = atomicAdd(count, (u32)__builtin_popcountll(mask));
    base = __shfl(base, leader, 64);
    return base + (u32)__builtin_popcountll(mask & lanemask_lt());
}
// the smallest v of the workgroup, in every lane (smem: NT / 64 words)
template <int NT>
LCP_DEVICE u32 lcp_block_min(u32 v, u32 *smem) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 t = __shfl_xor(v, d, 64);
        v = t < v ? t : v;
    }
    lcp_sync();
    if (lane_id() == 0) smem[threadIdx.x >> 6] = v;
    lcp_sync();
    u32 m = smem[0];
#pragma unroll
    for (int i = 1; i < NT / 64; i++) m = smem[i] < m ? smem[i] : m;
    return m;
}
// exclusive max-scan over the lanes of the workgroup (identity 0); *total = the workgroup's maximum (smem: NT / 64 words)
template <int NT>
LCP_DEVICE u32 lcp_block_excl_max(u32 v, u32 *smem, u32 *total) {
    const int w = threadIdx.x >> 6;
    const u32 inc = wave_incl_max(v);
    u32 ex = __shfl_up(inc, 1, 64);
    if (lane_id() == 0) ex = 0;
    lcp_sync();
    if (lane_id() == 63) smem[w] = inc;
    lcp_sync();
    u32 base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        const u32 s = smem[i];
        if (i < w) base = s > base ? s : base;
        tot = s > tot ? s : tot;
    }
    *total = tot;
    return ex > base ? ex : base;
}
// the workgroup's (key, sum) into out2[0] (max) and out2[1] (sum): one pair of atomics per workgroup (smem: 2 * NT / 64 words)
LCP_DEVICE void lcp_summary_publish(u64 key, u64 sum, u64 *smem, u64 *out2) {
    key = wave_max64(key);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { smem[2 * w] = key; smem[2 * w + 1] = sum; }
    lcp_sync();
    if (threadIdx.x == 0) {
        for (int i = 1; i < LCP_NT / 64; i++) {
            key = smem[2 * i] > key ? smem[2 * i] : key;
            sum += smem[2 * i + 1];
        }
        atomicMax((unsigned long long *)&out2[0], (unsigned long long)key);
        atomicAdd((unsigned long long *)&out2[1], (unsigned long long)sum);
    }
}
#endif

// ---- the comparison ----------------------------------------------------------------------------------------------
// 8 text bytes from any address, byte 0 in the low bits
LCP_DEVICE u64 lcp_load8(const u8 *p) {
    u64 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
// how many of the 16 bytes at a and at b agree before the first that differs (16: all)
LCP_DEVICE u32 lcp_match16(u64 a_lo, u64 a_hi, u64 b_lo, u64 b_hi) {
    const u64 x = a_lo ^ b_lo, y = a_hi ^ b_hi;
    if (x) return lcp_ctz64(x) >> 3;
    if (y) return 8 + (lcp_ctz64(y) >> 3);
    return 16;
}
// the same for r < 16 bytes, one at a time: the last bytes before the end of the text
LCP_DEVICE u32 lcp_match_bytes(const u8 *a, const u8 *b, u32 r) {
    u32 m = 0;
    while (m < r && a[m] == b[m]) m++;
    return m;
}

// ---- step 1 ------------------------------------------------------------------------------------------------------
// phi preset to LCP_UNSET (N words).  Row j >= 1 writes phi[sa[j]] = sa[j - 1]; a row above n is never an index and
// raises the flag.  Grid: N lanes.
LCP_KERNEL lcp_phi_kernel(const u32 *sa, u64 N, u32 n, u32 *phi, u32 *err) {
    const u64 j = (u64)lcp_bid() * LCP_NT + lcp_tid();
    if (j == 0 || j >= N) return;
    const u32 cur = sa[j], prev = sa[j - 1];
    if (cur > n || prev > n) {
        lcp_flag(err, LCP_ERR_SA);
        return;
    }
    phi[cur] = prev;
}

// ---- step 2 ------------------------------------------------------------------------------------------------------
// One lane per text position i in 0 .. n.  v[i] holds phi[i] on entry; on exit V[i]: 0 for a reducible or unset
// position, l + i for a finished comparison; an irreducible position whose comparison reached `cap` (a multiple of 16)
// with text left keeps phi[i] and goes to list[] (its final length is at least cap, so it needs no placeholder: step 3
// writes it before the scan reads it).  *count: slots drawn; the list holds list_cap of them -- for a suffix array at
// most 2 n log2 n / cap positions reach the cap, so a draw beyond list_cap proves that sa is none, and raises the flag.
LCP_KERNEL lcp_irreducible_kernel(const u8 *text, u32 n, const u32 *sa, u32 *v, u32 cap, u32 *list, u32 list_cap, u32 *count,
                                  u32 *err) {
    const u64 gi = (u64)lcp_bid() * LCP_NT + lcp_tid();
    const bool live = gi <= n;
    const u32 i = live ? (u32)gi : 0;
    bool is_long = false;
    if (live) {
        const u32 p = v[i];
        if (p == LCP_UNSET) {
            if (i != sa[0]) lcp_flag(err, LCP_ERR_SA);
            v[i] = 0;
        } else {
            const u32 lim = n - (i > p ? i : p);   // bytes both suffixes have
            const u32 L = lim < cap ? lim : cap;
            const u8 *a = text + i, *b = text + p;
            // the bytes in front and the first 16 of both sides, issued together
            const bool front = i > 0 && p > 0;
            const u32 fa = front ? a[-1] : 0x100u, fb = front ? b[-1] : 0x200u;
            u64 a0 = 0, a1 = 0, b0 = 0, b1 = 0;
            if (L >= 16) { a0 = lcp_load8(a); a1 = lcp_load8(a + 8); b0 = lcp_load8(b); b1 = lcp_load8(b + 8); }
            if (fa == fb) {
                v[i] = 0;   // reducible
            } else {
                u32 l = 0;
                bool open = true;   // no differing byte found yet
                if (L >= 16) {
                    const u32 m = lcp_match16(a0, a1, b0, b1);
                    l = m;
                    open = m == 16;
                }
                // two 16-byte steps a turn: four loads a side in flight
                while (open && l + 32 <= L) {
                    const u64 c0 = lcp_load8(a + l), c1 = lcp_load8(a + l + 8), c2 = lcp_load8(a + l + 16), c3 = lcp_load8(a + l + 24);
                    const u64 d0 = lcp_load8(b + l), d1 = lcp_load8(b + l + 8), d2 = lcp_load8(b + l + 16), d3 = lcp_load8(b + l + 24);
                    u32 m = lcp_match16(c0, c1, d0, d1);
                    if (m == 16) m += lcp_match16(c2, c3, d2, d3);
                    l += m;
                    open = m == 32;
                }
                if (open && l + 16 <= L) {
                    const u32 m = lcp_match16(lcp_load8(a + l), lcp_load8(a + l + 8), lcp_load8(b + l), lcp_load8(b + l + 8));
                    l += m;
                    open = m == 16;
                }
                if (open && l < L) {   // fewer than 16 bytes to L: only when the text ends before the cap
                    const u32 m = lcp_match_bytes(a + l, b + l, L - l);
                    l += m;
                }
                if (l >= cap && l < lim) is_long = true;
                else v[i] = l + i;
            }
        }
    }
    const u32 slot = lcp_wave_append(is_long, count);
    if (is_long) {
        if (slot < list_cap) list[slot] = i;
        else lcp_flag(err, LCP_ERR_SA);
    }
}

// ---- step 3 ------------------------------------------------------------------------------------------------------
// One workgroup per long item, items taken round robin.  A turn covers 2 * act chunks of 16 bytes from offset l on: chunk
// c = u * act + lane, so that the lanes of one load are neighbours; every lane answers how many bytes of its chunks agree
// and the smallest offset at which one stops is the workgroup's.  act = the lanes that load in this turn: one wave in
// the first, two in the second, then all (2, 4, 8 KiB a side), so that a value a few bytes above the cap costs one wave's
// loads, not the workgroup's.  A chunk that would pass the end of both suffixes (lim) is compared byte by byte up to
// lim, and stops there.
LCP_KERNEL lcp_long_kernel(const u8 *text, u32 n, u32 *v, u32 cap, const u32 *list, u32 list_cap, const u32 *count) {
    LCP_SHARED u32 smem[LCP_NT / 64 + 1];
    u32 items = lcp_load_u32(count);
    if (items > list_cap) items = list_cap;
    for (u32 k = lcp_bid(); k < items; k += lcp_nblocks()) {
        const u32 i = list[k];
        if (i > n) continue;        // (never: step 2 wrote it)
        const u32 p = v[i];
        if (p > n) continue;        // (never: an item keeps its phi, and step 1 stores no value above n)
        const u32 lim = n - (i > p ? i : p);
        const u8 *a = text + i, *b = text + p;
        u64 l = cap < lim ? cap : lim;   // (u64: l + step may pass 2^32)
        for (u32 turn = 0;; turn++) {
            const u32 act = turn < 2 && (64u << turn) < LCP_NT ? 64u << turn : LCP_NT;
            const u32 step = 2u * act * 16u;
            const bool on = lcp_tid() < act;
            const u64 o0 = l + (u64)lcp_tid() * 16u, o1 = o0 + (u64)act * 16u;
            const bool w0 = on && o0 + 16 <= lim, w1 = on && o1 + 16 <= lim;
            u64 a0 = 0, a1 = 0, b0 = 0, b1 = 0, a2 = 0, a3 = 0, b2 = 0, b3 = 0;
            if (w0) { a0 = lcp_load8(a + o0); a1 = lcp_load8(a + o0 + 8); b0 = lcp_load8(b + o0); b1 = lcp_load8(b + o0 + 8); }
            if (w1) { a2 = lcp_load8(a + o1); a3 = lcp_load8(a + o1 + 8); b2 = lcp_load8(b + o1); b3 = lcp_load8(b + o1 + 8); }
            u32 m0, m1;
            if (w0) m0 = lcp_match16(a0, a1, b0, b1);
            else m0 = on && o0 < lim ? lcp_match_bytes(a + o0, b + o0, (u32)(lim - o0)) : 0;
            if (w1) m1 = lcp_match16(a2, a3, b2, b3);
            else m1 = on && o1 < lim ? lcp_match_bytes(a + o1, b + o1, (u32)(lim - o1)) : 0;
            // offset within the turn at which this lane's chunks stop (step: they do not)
            u32 stop = step;
            if (on && m1 < 16) stop = (u32)(o1 - l) + m1;
            if (on && m0 < 16) stop = (u32)(o0 - l) + m0;
            stop = lcp_block_min<LCP_NT>(stop, smem);
            l += stop;
            if (stop < step) break;
        }
        if (lcp_tid() == 0) v[i] = (u32)l + i;   // l <= lim: the sum is at most n
    }
}

// ---- step 4 ------------------------------------------------------------------------------------------------------
// Inclusive max-scan of v[0 .. N) in place, tiles of LCP_SCAN_NT * LCP_SCAN_ITEMS values: (a) the maximum of every tile,
// (b) one workgroup turns tmax[0 .. ntiles) into its exclusive scan, (c) every tile scans itself above its carry.
#define LCP_SCAN_TILE (LCP_SCAN_NT * LCP_SCAN_ITEMS)
LCP_KERNEL lcp_scan_reduce_kernel(const u32 *v, u64 N, u32 *tmax) {
    LCP_SHARED u32 smem[LCP_SCAN_NT / 64 + 1];
    const u64 base = (u64)lcp_bid() * LCP_SCAN_TILE;
    u32 m = 0;
#pragma unroll
    for (int k = 0; k < LCP_SCAN_ITEMS; k++) {   // lane-interleaved: a maximum does not care for the order
        const u64 idx = base + (u64)k * LCP_SCAN_NT + lcp_tid();
        const u32 x = idx < N ? v[idx] : 0;
        m = x > m ? x : m;
    }
    u32 total;
    (void)lcp_block_excl_max<LCP_SCAN_NT>(m, smem, &total);
    if (lcp_tid() == 0) tmax[lcp_bid()] = total;
}
// one workgroup: every lane takes `per` consecutive tiles
LCP_KERNEL lcp_scan_tiles_kernel(u32 *tmax, u32 ntiles, u32 per) {
    LCP_SHARED u32 smem[LCP_SCAN_NT / 64 + 1];
    const u64 lo = (u64)lcp_tid() * per;
    u64 hi = lo + per;
    if (hi > ntiles) hi = ntiles;
    u32 m = 0;
    for (u64 t = lo; t < hi; t++) m = tmax[t] > m ? tmax[t] : m;
    u32 total;
    u32 carry = lcp_block_excl_max<LCP_SCAN_NT>(m, smem, &total);
    for (u64 t = lo; t < hi; t++) {
        const u32 x = tmax[t];
        tmax[t] = carry;
        carry = x > carry ? x : carry;
    }
}
LCP_KERNEL lcp_scan_apply_kernel(u32 *v, u64 N, const u32 *tcarry) {
    LCP_SHARED u32 smem[LCP_SCAN_NT / 64 + 1];
    const u64 base = (u64)lcp_bid() * LCP_SCAN_TILE + (u64)lcp_tid() * LCP_SCAN_ITEMS;   // a multiple of 16 words: 64-byte lines
    u32 x[LCP_SCAN_ITEMS];
    const bool full = base + LCP_SCAN_ITEMS <= N;
    if (full) {
#pragma unroll
        for (int k = 0; k < LCP_SCAN_ITEMS; k += 4) __builtin_memcpy(&x[k], __builtin_assume_aligned(v + base + k, 16), 16);
    } else {
#pragma unroll
        for (int k = 0; k < LCP_SCAN_ITEMS; k++) x[k] = base + k < N ? v[base + k] : 0;
    }
#pragma unroll
    for (int k = 1; k < LCP_SCAN_ITEMS; k++) x[k] = x[k] > x[k - 1] ? x[k] : x[k - 1];
    u32 total;
    u32 carry = lcp_block_excl_max<LCP_SCAN_NT>(x[LCP_SCAN_ITEMS - 1], smem, &total);
    const u32 tc = tcarry[lcp_bid()];
    carry = tc > carry ? tc : carry;
#pragma unroll
    for (int k = 0; k < LCP_SCAN_ITEMS; k++) x[k] = x[k] > carry ? x[k] : carry;
    if (full) {
#pragma unroll
        for (int k = 0; k < LCP_SCAN_ITEMS; k += 4) __builtin_memcpy(__builtin_assume_aligned(v + base + k, 16), &x[k], 16);
    } else {
#pragma unroll
        for (int k = 0; k < LCP_SCAN_ITEMS; k++)
            if (base + k < N) v[base + k] = x[k];
    }
}

// ---- step 5 ------------------------------------------------------------------------------------------------------
// Row order again: lcp[j] = scan[sa[j]] - sa[j], never below 0 and never above n - max(sa[j - 1], sa[j]) (both hold by
// themselves for a suffix array; for any other permutation they keep the value within the header's promise).  A row
// above n is no index: 0.  Grid: N lanes.
LCP_KERNEL lcp_gather_kernel(const u32 *sa, u64 N, u32 n, const u32 *scan, u32 *lcp) {
    const u64 j = (u64)lcp_bid() * LCP_NT + lcp_tid();
    if (j >= N) return;
    u32 out = 0;
    if (j > 0) {
        const u32 cur = sa[j], prev = sa[j - 1];
        if (cur <= n && prev <= n) {
            const u32 s = scan[cur];
            const u32 bound = n - (cur > prev ? cur : prev);
            out = s > cur ? s - cur : 0;
            out = out < bound ? out : bound;
        }
    }
    lcp[j] = out;
}

// ---- tc_lcp_summary_dev --------------------------------------------------------------------------------------------
// out2[0] = max over rows of (lcp << 32 | ~row): the largest value, and of its rows the smallest; out2[1] = the sum.
// Both zeroed before the launch.  Any grid: the lanes stride over the rows.
LCP_KERNEL lcp_summary_kernel(const u32 *lcp, u64 N, u64 *out2) {
    LCP_SHARED u64 smem[2 * (LCP_NT / 64) + 2];
    u64 key = 0, sum = 0;
    const u64 stride = (u64)lcp_nblocks() * LCP_NT;
    for (u64 j = (u64)lcp_bid() * LCP_NT + lcp_tid(); j < N; j += stride) {
        const u32 x = lcp[j];
        const u64 k = ((u64)x << 32) | (u64)(0xffffffffu - (u32)j);
        key = k > key ? k : key;
        sum += x;
    }
    lcp_summary_publish(key, sum, smem, out2);
}
