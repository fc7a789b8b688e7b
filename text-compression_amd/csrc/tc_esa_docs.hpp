// tc_esa_docs.hpp -- document collections on the kept enhanced suffix array: the document array and the array of previous rows
// of one document, their build, and document frequency and document listing of substrings of the text (included by
// tc_esa_docs_host.hpp behind tc_esa_host.hpp; it uses the min tree and the row searches of tc_fm_ms.hpp unchanged; DESIGN.md
// section 4.16).  No counterpart in the reference.  host/check/esa_docs_kernels.cpp compiles esd_doc_of, esd_doc_kernel and the lane
// bodies of the k-mer document frequency -- kmd_flags16, kmd_prefix, kmd_group_df -- as plain C++ (TC_FM_MS_HOST_CHECK, as
// tc_fm_ms.hpp describes); the build's kernels, the workgroup scans and the tile kernels around the lane bodies exist on the device
// only.
//
// include/textcomp.h defines the answers.  The text is the concatenation of ndocs documents, doc_start[0 .. ndocs] their
// boundaries; position p belongs to the document d with doc_start[d] <= p < doc_start[d + 1], an occurrence to the document of
// its first byte.  Over the N = n + 1 rows of the handle:
//   da[r]   the document of sa[r]; ESD_NO_DOC for the empty suffix (row 0)
//   pv[r]   1 + the largest row r' < r with da[r'] = da[r], 0 where there is none; pv[0] = 0xffffffff
//   P       the min tree of pv, of the handle's shape
// For the rows [lo, hi) of a substring, lo >= 1, the rows x with pv[x] <= lo are one row per distinct document, that document's
// first row of the interval (Muthukrishnan's document listing).  "The smallest row > b with pv[row] < lo + 1" is fm_ms_next_below
// over P, so a query is the two row searches of find and then one such search per document found: no stack, at most 2 f words
// per level and step on any text.  The loop ends at hi, at `limit`, and after ndocs steps -- finite on ANY contents of pv and of
// its tree; every row it reads is below hi <= N.  An isa entry that is no row (no build writes one) gives an empty interval:
// the outputs are written, 0 documents.
// The build: da by a binary search of sa[r] in doc_start, one lane per row (the table in LDS while it fits); pv from the rows in
// (document, row) order, which is a stable LSD sort of r = 0 .. N - 1 by the key da[r] + 1 (0 .. ndocs: one pass of 8 bits up to
// 255 documents, two above).  A pass is three kernels -- the tiles' digit counts, the scan of the counts (digit-major, so one
// exclusive scan gives every tile's first slot of every digit), the scatter, which ranks a tile's items by ballots, stripe by
// stripe of 64 consecutive items per wave -- and none of them waits on another workgroup.  Then each item looks at its
// predecessor.
#pragma once
#include "tc_esa.hpp"
#if defined(TC_FM_MS_HOST_CHECK) && !defined(TC_KM_HOST_CHECK)
#define TC_KM_HOST_CHECK
#endif
#include "tc_kmer.hpp"

#define ESD_NO_DOC 0xffffffffu      // TC_ESA_NO_DOC of include/textcomp.h
#define ESD_MAX_DOCS 65535u         // TC_ESA_MAX_DOCS

#ifdef TC_FM_MS_HOST_CHECK
// what host/check/esa_docs_kernels.cpp asserts happened: the loop ended [0] at hi, [1] at limit, [2] after ndocs steps, [3] at the
// end of its segment (fill); [4] len = 0, [5] a query refused, [6] a first row of 0 clamped (not on a suffix array)
static u64 esd_seen[7] = {};
#define ESD_SEEN(k) (esd_seen[k]++)
#else
#define ESD_SEEN(k) ((void)0)
#endif

// the document of position p: the d with ds[d] <= p < ds[d + 1] (ds[0] = 0, non-decreasing, ds[ndocs] = n); ESD_NO_DOC for p >= n
FM_MS_DEVICE u32 esd_doc_of(const u32 *ds, u32 ndocs, u32 p) {
    if (p >= ds[ndocs]) return ESD_NO_DOC;
    u32 lo = 1, hi = ndocs;             // the smallest j in [1, ndocs] with ds[j] > p: ndocs qualifies
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (ds[mid] > p) hi = mid;
        else lo = mid + 1u;
    }
    return lo - 1u;
}

// One lane per query q < nq over the substring text[start .. start + len).  The count instance: df[q] = the number of distinct
// documents with an occurrence, at most `limit` where limit > 0 (u32; may be null), occ[q] as esa_find_kernel (may be null), cnt[q]
// = df[q] as 64 bits for the scan (may be null).  The fill instance: the documents, in the order of their first row x in the
// interval, go to docs[offs[q] + i], sa[x] to hit_pos (may be null), at most offs[q + 1] - offs[q] of them.  len = 0: the rows
// [1, N), every non-empty document.
template <bool FILL>
FM_MS_KERNEL esd_doc_kernel(u32 n, const u32 *__restrict__ sa, const u32 *__restrict__ isa, const u32 *__restrict__ lcp,
                            const u32 *__restrict__ lcp_min, const u32 *__restrict__ da, const u32 *__restrict__ pv,
                            const u32 *__restrict__ pv_min, u32 lf, u32 ndocs, const u32 *__restrict__ qs, const u32 *__restrict__ ql,
                            u64 nq, u32 limit, u32 *__restrict__ df, u32 *__restrict__ occ, u64 *__restrict__ cnt,
                            const u64 *__restrict__ offs, u32 *__restrict__ docs, u32 *__restrict__ hit_pos, u32 *__restrict__ bad) {
    const u32 N = n + 1u;
    ESA_TREE_SHAPE(N, lf);
    const u64 q = (u64)fm_ms_bid() * FM_MS_NT + fm_ms_tid();
    if (q >= nq) return;
    const u32 s = qs[q], l = ql[q];
    if (s > n || l > n - s) {
        ESD_SEEN(5);
        bad[0] = 1u;
        return;
    }
    FmMsTree T;
    T.lcp = lcp; T.lmin = lcp_min; T.s_off = s_off; T.s_cnt = s_cnt; T.nlev = s_nlev; T.lf = lf;
    u32 lo = 1u, hi = N;
    if (l) {
        const u32 r = isa[s];                       // (s < n: l >= 1)
        if (r < N) {
            lo = fm_ms_prev_below(T, r, l);
            hi = fm_ms_next_below(T, N, r, l);
        } else {                                    // (not on an inverse suffix array: no row, no document -- the outputs are written)
            hi = lo;
        }
        if (lo == 0) {                              // (row 0 is the empty suffix and starts with no byte: not on a suffix array)
            ESD_SEEN(6);
            lo = 1u;
        }
    } else {
        ESD_SEEN(4);
    }
    const u32 width = l ? hi - lo : N;
    T.lcp = pv; T.lmin = pv_min;
    u64 o = 0;
    u32 room = 0xffffffffu;
    if (FILL) {
        o = offs[q];
        const u64 have = offs[q + 1] - o;
        room = have < 0xffffffffull ? (u32)have : 0xffffffffu;
    }
    u32 c = 0, b = lo - 1u;
    while (true) {
        if (limit && c == limit) {
            ESD_SEEN(1);
            break;
        }
        if (c == ndocs) {                           // (a document has one first row: keeps the loop finite on any content)
            ESD_SEEN(2);
            break;
        }
        if (FILL && c == room) {
            ESD_SEEN(3);
            break;
        }
        const u32 x = fm_ms_next_below(T, N, b, lo + 1u);
        if (x >= hi) {
            ESD_SEEN(0);
            break;
        }
        if (FILL) {
            docs[o + c] = da[x];
            if (hit_pos) hit_pos[o + c] = sa[x];
        }
        c++;
        b = x;
    }
    if (!FILL) {
        if (df) df[q] = c;
        if (occ) occ[q] = width;
        if (cnt) cnt[q] = c;
    }
}

// ---- the lane bodies of the k-mer document frequency (the kernels and the method: below, behind the build's kernels)
// bit i: row base + i is FLAGGED, pv[row] <= head(row).  mask: the lane's boundaries (km_mask16), w[i] = pv[base + i] for the rows
// below N (the others are not looked at), prev1: the last boundary before the lane's rows, + 1 (0: none -- before row 0 only)
KM_HD u32 kmd_flags16(u32 mask, const u32 *w, u64 base, u64 N, u32 prev1) {
    u32 h1 = prev1;                             // the head of the row at hand, + 1 (rows are below 2^32)
    u32 fmask = 0;
    for (u32 i = 0; i < KM_ROWS; i++) {
        const u64 r = base + i;
        if ((mask >> i) & 1u) h1 = (u32)r + 1u;
        const bool f = r >= 1 && r < N && w[i] < h1;        // pv[r] <= head(r)
        fmask |= (f ? 1u : 0u) << i;
    }
    return fmask;
}
// the flags of the tile before its row xl (0 .. KM_TILE - 1); lbase[j]: the flags of the lanes before lane j, fmask[j]: its own
KM_HD u32 kmd_prefix(const u32 *lbase, const u32 *fmask, u32 xl) {
    return lbase[xl / KM_ROWS] + (u32)__builtin_popcount(fmask[xl / KM_ROWS] & ((1u << (xl % KM_ROWS)) - 1u));
}
// df of the group [row, row + occ) whose end lies in the tile at tile_base: F[end] - F[row], F[x] = fbase[tile of x] + the flags of
// that tile before x; a row before the tile is the last boundary of its own tile, where inlast has them
KM_HD u32 kmd_group_df(u32 row, u32 occ, u64 tile_base, const u32 *lbase, const u32 *fmask, const u64 *fbase, const u32 *inlast) {
    const u64 t = tile_base / KM_TILE;
    const u64 fq = fbase[t] + kmd_prefix(lbase, fmask, (u32)((u64)row + occ - tile_base));
    const u64 fp = row >= tile_base ? fbase[t] + kmd_prefix(lbase, fmask, (u32)(row - tile_base)) : fbase[row / KM_TILE] + inlast[row / KM_TILE];
    return (u32)(fq - fp);
}

#ifndef TC_FM_MS_HOST_CHECK
#define ESD_NT 256
#define ESD_ITEMS 16
#define ESD_TILE 4096           // = ESD_NT * ESD_ITEMS items per tile of the sort (tests/test_gpu_esa_docs.py states the same number)
#define ESD_LDS_DOCS 8192u      // doc_start entries kept in LDS by esd_da_kernel: 32 KB

// da[r] = the document of sa[r], one lane per row; LDS: the ndocs + 1 entries of doc_start go through dynamic LDS
template <bool LDS>
__global__ __launch_bounds__(ESD_NT) void esd_da_kernel(const u32 *__restrict__ sa, u64 N, const u32 *__restrict__ ds, u32 ndocs,
                                                        u32 *__restrict__ da) {
    extern __shared__ u32 esd_s_ds[];
    if (LDS) {
        for (u32 i = threadIdx.x; i <= ndocs; i += ESD_NT) esd_s_ds[i] = ds[i];
        __syncthreads();
    }
    const u64 r = (u64)blockIdx.x * ESD_NT + threadIdx.x;
    if (r >= N) return;
    da[r] = esd_doc_of(LDS ? esd_s_ds : ds, ndocs, sa[r]);
}

// An item of the sort: key << 32 | row, key = da[row] + 1 (0: no document).  GEN: the first pass makes its items from da.
template <bool GEN>
__device__ __forceinline__ u64 esd_item(const u32 *__restrict__ da, const u64 *__restrict__ in, u64 i) {
    return GEN ? (u64)(u32)(da[i] + 1u) << 32 | i : in[i];
}
__device__ __forceinline__ u32 esd_digit(u64 item, u32 shift) { return (u32)(item >> (32u + shift)) & 255u; }

// the lanes of the wave whose item has the digit d of this lane (valid lanes only), by 8 ballots
__device__ __forceinline__ u64 esd_match(u32 d, bool valid) {
    u64 m = __ballot(valid);
#pragma unroll
    for (u32 bit = 0; bit < 8; bit++) {
        const bool on = (d >> bit) & 1u;
        const u64 bal = __ballot(on);
        m &= on ? bal : ~bal;
    }
    return m;
}

// cnt[d * ntiles + t] = the items of tile t whose digit is d: digit-major, so that one exclusive scan of the whole array gives
// every tile's first slot of every digit.  Per stripe of 64 items the first lane of every digit adds its group: one LDS add per
// distinct digit and stripe, not one per item -- with one document every lane of a wave has the same digit
template <bool GEN>
__global__ __launch_bounds__(ESD_NT) void esd_sort_count_kernel(const u32 *__restrict__ da, const u64 *__restrict__ in, u64 N, u32 shift,
                                                                u64 *__restrict__ cnt) {
    __shared__ u32 s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * ESD_TILE + (u64)(threadIdx.x >> 6) * (64 * ESD_ITEMS) + (threadIdx.x & 63u);
#pragma unroll
    for (u32 k = 0; k < ESD_ITEMS; k++) {
        const u64 i = base + (u64)k * 64;
        const bool valid = i < N;
        const u32 d = valid ? esd_digit(esd_item<GEN>(da, in, i), shift) : 0u;
        const u64 m = esd_match(d, valid);
        if (valid && (m & lanemask_lt()) == 0) atomicAdd(&s_h[d], (u32)__popcll(m));
    }
    __syncthreads();
    cnt[(u64)threadIdx.x * gridDim.x + blockIdx.x] = s_h[threadIdx.x];
}

// The scatter of one pass, stable: wave w takes the tile's items [1024 w, 1024 w + 1024) in 16 stripes of 64 consecutive ones;
// within a stripe the lanes of one digit find each other by 8 ballots, the lanes before a lane in its group are its rank, and the
// group's first lane adds the group to the wave's count of the digit.  offs: the scan of esd_sort_count_kernel's counts.
template <bool GEN>
__global__ __launch_bounds__(ESD_NT) void esd_sort_scatter_kernel(const u32 *__restrict__ da, const u64 *__restrict__ in, u64 N, u32 shift,
                                                                  const u64 *__restrict__ offs, u64 *__restrict__ out) {
    __shared__ u32 s_wh[ESD_NT / 64][256];
    __shared__ u64 s_first[ESD_NT / 64][256];
    const u32 w = threadIdx.x >> 6;
    for (u32 i = 0; i < ESD_NT / 64; i++) s_wh[i][threadIdx.x] = 0;
    __syncthreads();
    volatile u32 *wh = s_wh[w];
    const u64 base = (u64)blockIdx.x * ESD_TILE + (u64)w * (64 * ESD_ITEMS) + (threadIdx.x & 63u);
    u64 item[ESD_ITEMS];
    u32 rnk[ESD_ITEMS];
#pragma unroll
    for (u32 k = 0; k < ESD_ITEMS; k++) {
        const u64 i = base + (u64)k * 64;
        const bool valid = i < N;
        item[k] = valid ? esd_item<GEN>(da, in, i) : 0;
        const u32 d = esd_digit(item[k], shift);
        const u64 m = esd_match(d, valid);
        const u32 prior = (u32)__popcll(m & lanemask_lt());
        const u32 old = valid ? wh[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && prior == 0) wh[d] = old + (u32)__popcll(m);
        __builtin_amdgcn_wave_barrier();
        rnk[k] = old + prior;
    }
    __syncthreads();
    {   // one lane per digit: where each wave's items of the digit start
        u64 run = offs[(u64)threadIdx.x * gridDim.x + blockIdx.x];
        for (u32 i = 0; i < ESD_NT / 64; i++) {
            s_first[i][threadIdx.x] = run;
            run += s_wh[i][threadIdx.x];
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < ESD_ITEMS; k++) {
        const u64 i = base + (u64)k * 64;
        if (i < N) out[s_first[w][esd_digit(item[k], shift)] + rnk[k]] = item[k];
    }
}

// items in (document, row) order: each row's predecessor of its document is the item before it
__global__ __launch_bounds__(ESD_NT) void esd_pv_kernel(const u64 *__restrict__ items, u64 N, u32 *__restrict__ pv) {
    const u64 i = (u64)blockIdx.x * ESD_NT + threadIdx.x;
    if (i >= N) return;
    const u64 it = items[i];
    const u32 key = (u32)(it >> 32), row = (u32)it;     // (row < N: the first pass made it from an index)
    u32 v = 0xffffffffu;
    if (key) {
        v = 0;
        if (i) {
            const u64 before = items[i - 1];
            if ((u32)(before >> 32) == key) v = (u32)before + 1u;
        }
    }
    pv[row] = v;
}

// ---- the document frequency of every k-mer: the groups of tc_kmer.hpp (tiles of KM_NT lanes x KM_ROWS rows, boundary masks,
// heads by a max scan within the tile and carries across tiles) partition the rows, and df(group [p, q)) = #{r in [p, q) :
// pv[r] <= p}.  Row r is FLAGGED iff pv[r] <= head(r), the last boundary at or before r; with F the exclusive prefix sum of the
// flags over all rows, df = F[q] - F[p].  F[x] = fbase[t] + the flags of tile t before x: kmd_flag_kernel writes every tile's
// flag total (their scan is fbase) and the flags before its last boundary row (inlast) -- a head p that lies before the tile of
// q is the last boundary of its own tile, so F[p] = fbase[tp] + inlast[tp] -- and kmd_pass_kernel looks the prefix of a row of
// its own tile up in LDS (every lane's first prefix and its 16 flag bits).  No lane walks a group: a unary text, one group
// over every tile, and a text of all-distinct k-mers cost the same passes.  Every read of pv is of a row below N and its value is
// only compared: the passes stay in bounds on any contents of the arrays.
struct KmdLane {
    u32 mask, prev1, cr, fmask, tile_last, lbase, ftotal;
};
// one lane's part of a tile: its boundary mask and head as km_pass_kernel has them, its 16 flags, and the tile's tables in LDS
// (s_scan: KM_NT / 64 + 1 words, s_lbase and s_fmask: KM_NT words each); ends with a barrier
__device__ __forceinline__ KmdLane kmd_lane(const u32 *__restrict__ lcp, const u32 *__restrict__ pv, u64 N, u32 k, u32 aligned,
                                            const u32 *__restrict__ carry, u32 *s_scan, u32 *s_lbase, u32 *s_fmask) {
    KmdLane L;
    const u64 base = (u64)blockIdx.x * KM_TILE + (u64)threadIdx.x * KM_ROWS;
    u32 w[KM_ROWS];
    km_load16(lcp, base, N, (aligned & 1u) != 0, w);
    L.mask = km_mask16(w, base, N, k);
    L.prev1 = km_block_excl_max(km_last1(L.mask, base), s_scan, &L.tile_last);
    L.cr = carry[blockIdx.x];
    L.prev1 = L.prev1 > L.cr ? L.prev1 : L.cr;
    km_load16(pv, base, N, (aligned & 2u) != 0, w);
    L.fmask = kmd_flags16(L.mask, w, base, N, L.prev1);
    L.lbase = block_excl_sum<KM_NT>((u32)__popc(L.fmask), s_scan, &L.ftotal);
    s_lbase[threadIdx.x] = L.lbase;
    s_fmask[threadIdx.x] = L.fmask;
    __syncthreads();
    return L;
}

// fsum[t] = the flags of tile t; inlast[t] = those before its last boundary row (0 where the tile has no boundary)
__global__ __launch_bounds__(KM_NT, 8) void kmd_flag_kernel(const u32 *__restrict__ lcp, const u32 *__restrict__ pv, u64 N, u32 k, u32 aligned,
                                                         const u32 *__restrict__ carry, u64 *__restrict__ fsum, u32 *__restrict__ inlast) {
    __shared__ u32 s_scan[KM_NT / 64 + 1], s_lbase[KM_NT], s_fmask[KM_NT];
    const KmdLane L = kmd_lane(lcp, pv, N, k, aligned, carry, s_scan, s_lbase, s_fmask);
    if (threadIdx.x == 0) {
        const u64 tile_base = (u64)blockIdx.x * KM_TILE;
        fsum[blockIdx.x] = L.ftotal;
        inlast[blockIdx.x] = L.tile_last ? kmd_prefix(s_lbase, s_fmask, (u32)((u64)L.tile_last - 1u - tile_base)) : 0u;
    }
}

// The groups that END in tile t, with their document frequency.  COUNT: cnt[t] = how many pass min_df <= df (and df <= max_df
// unless max_df = 0).  FILL: they go to pos / occ / df / row (each may be null) from slot offs[t] on, in row order, through LDS
// (one packed word per k-mer; df is computed again where it is stored), no atomics.  HIST: hist[min(df, bins - 1)] += 1 for every k-mer, the first min(bins, KM_LDS_BINS) bins through LDS as
// km_pass_kernel's spectrum; *distinct gets the tile's count.
template <int MODE>
__global__ __launch_bounds__(KM_NT, 8) void kmd_pass_kernel(const u32 *__restrict__ sa, const u32 *__restrict__ lcp, const u32 *__restrict__ pv,
                                                         u64 N, u32 k, u32 min_df, u32 max_df, u32 aligned, const u32 *__restrict__ carry,
                                                         const u64 *__restrict__ fbase, const u32 *__restrict__ inlast,
                                                         u64 *__restrict__ cnt, const u64 *__restrict__ offs, u32 *__restrict__ kpos,
                                                         u32 *__restrict__ kocc, u32 *__restrict__ kdf, u32 *__restrict__ krow,
                                                         u64 *__restrict__ hist, u32 bins, u64 *__restrict__ distinct) {
    __shared__ u32 s_scan[KM_NT / 64 + 1], s_lbase[KM_NT], s_fmask[KM_NT];
    __shared__ u32 s_hist[MODE == KM_HIST ? KM_LDS_BINS : 1];
    __shared__ u32 s_stage[MODE == KM_FILL ? KM_TILE : 1];
    const u64 n = N - 1u;
    const u64 tile_base = (u64)blockIdx.x * KM_TILE, base = tile_base + (u64)threadIdx.x * KM_ROWS;
    const u32 lds_bins = bins < KM_LDS_BINS ? bins : KM_LDS_BINS;
    if (MODE == KM_HIST) {
        for (u32 i = threadIdx.x; i < lds_bins; i += KM_NT) s_hist[i] = 0;   // (the barriers of kmd_lane order this before the adds)
    }
    const KmdLane L = kmd_lane(lcp, pv, N, k, aligned, carry, s_scan, s_lbase, s_fmask);
    auto df_of = [&](u32 row, u32 occ) { return kmd_group_df(row, occ, tile_base, s_lbase, s_fmask, fbase, inlast); };
    auto passes = [&](u32 df) { return df >= min_df && (max_df == 0 || df <= max_df); };
    u32 c = 0;
    if (MODE == KM_HIST) {
        c = km_lane_close(L.mask, base, L.prev1, sa, n, k, 1u, 0u, [&](u32, u32 row, u32, u32 occ) {
            const u32 df = df_of(row, occ);
            const u32 b = df < bins ? df : bins - 1u;
            if (b < lds_bins) atomicAdd(&s_hist[b], 1u);
            else atomicAdd(reinterpret_cast<unsigned long long *>(hist + b), 1ull);
        });
    } else {
        km_lane_close(L.mask, base, L.prev1, sa, n, k, 1u, 0u, [&](u32, u32 row, u32, u32 occ) { c += passes(df_of(row, occ)) ? 1u : 0u; });
    }
    u32 total;
    const u32 before = block_excl_sum<KM_NT>(c, s_scan, &total);
    if (MODE == KM_COUNT) {
        if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    } else if (MODE == KM_FILL) {
        if (c) {
            u32 j = 0;
            km_lane_close(L.mask, base, L.prev1, sa, n, k, 1u, 0u, [&](u32, u32 row, u32, u32 occ) {
                if (!passes(df_of(row, occ))) return;
                const u32 ql = (u32)((u64)row + occ - tile_base);
                const u32 pl = row >= tile_base ? (u32)(row - tile_base) : 0xffffu;
                s_stage[before + j] = ql << 16 | pl;
                j++;
            });
        }
        __syncthreads();
        const u64 o = offs[blockIdx.x];
        for (u32 i = threadIdx.x; i < total; i += KM_NT) {
            const u32 v = s_stage[i];
            const u64 q = tile_base + (v >> 16);
            const u64 p = (v & 0xffffu) == 0xffffu ? (u64)L.cr - 1u : tile_base + (v & 0xffffu);
            if (kpos) kpos[o + i] = sa[p];
            if (kocc) kocc[o + i] = (u32)(q - p);
            if (kdf) kdf[o + i] = df_of((u32)p, (u32)(q - p));     // (again: a staged df would cost the tile 16 KB of LDS more)
            if (krow) krow[o + i] = (u32)p;
        }
    } else {
        __syncthreads();
        for (u32 i = threadIdx.x; i < lds_bins; i += KM_NT) {
            const u32 v = s_hist[i];
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(hist + i), (unsigned long long)v);
        }
        if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long *>(distinct), (unsigned long long)total);
    }
}
#endif  // TC_FM_MS_HOST_CHECK
