// tc_sa_host.hpp -- host driver of the suffix sort: sa_build carves the workspace and runs sa_run, a sequence of named
// phases over one SaRun (alphabet, round 0 by the MSD or the LSD way or the full path, rank tables, doubling rounds).
// The decisions that need no device are in tc_sa_plan.hpp.  Included by tc_encode_host.hpp only.
#pragma once
#include <chrono>

#include "tc_sa_plan.hpp"

// ------------------------------------------------------------------ suffix array
#ifndef SA_KDIR_BITS
#define SA_KDIR_BITS 26
#endif
// Buffers that serve a second purpose while their first one is idle:
//   hist          the region cursor of rank_cursor_kernel / rank_bin_kernel (free between the radix passes of two
//                 rounds), and the counters of the trace's group-size and chain diagnostics
//   act[1]        round 0 appends the tied set to 64 regions of it, which are then packed into act[0]; after that its
//                 slot + idx arrays (adjacent in the arena, together N u64) are the partition scratch of the ranks by
//                 regions, and its slot array the over-long-bucket bitmap of the tier-2 fix pass
//   msd_seg[last] once the last level's segment table is dead: the list of whole buckets (2 * 2^20 words), behind it
//                 the finish kernel's lut
//   chain_ref     once a chain round's flags are made the reference table is dead: the saved on-path and sign bitmaps
//                 go there (they must survive the sort of pass 1)
//   seg.segbits,  a chain round's on-path and sign flags while they are made (the segmented sort writes both anew)
//   seg.ybits
//   v0            key-only MSD levels move no values: out_khi of the finish (key bits 40..63 of every tied member)
//   k0 / k1       whichever does not hold the sorted round-0 keys is the pair scratch of the dense ranks; in dense
//                 mode both are dead after the ranks and carry the doubling rounds' keys
struct SaBuffers {
    u64 *k0, *k1;
    u32 *v0, *v1;
    u32 *isa;
    u32 *v2;
    u32 *act[2][4];  // [set][slot, idx, grp, tpos]
    // sparse mode (few tied suffixes): round buffers + rank table, each `sparse_cap` long
    u64 *sk[2];
    u32 *sv[2];
    u32 *t_idx, *t_rank;
    u64 *t_bits;   // N bits
    u32 *t_dir;    // per 64-bit word of t_bits
    u32 *t_bsum;
    u32 *fin_rc;   // finish_kernel: region counters + region offsets
    u32 *kdir;     // 2^SA_KDIR_BITS + 1
    u64 sparse_cap;
    u32 *hist;
    u64 *rstatus;
    u64 *gstatus;  // 2*tiles + 2
    u32 *counts;   // 256 byte counts
    // MSD round 0 (tc_msd.hpp), carved only for texts long enough to take it
    u32 *msd_pstart[MSD_LEVELS + 1], *msd_pcnt[MSD_LEVELS + 1];   // [l]: parents of level l + 1; [3]: level-3 buckets
    u32 *msd_tpre[MSD_LEVELS], *msd_seg[MSD_LEVELS];
    u32 *msd_joint;   // [256^3] child counts of the level-3 parents, gathered by the level-2 counting pass
    u32 msd_grid;
    TiedTable tp;     // key-only levels: hash table of the tied keys (tc_sa.hpp)
    SegBuffers seg;   // segmented sort of the doubling rounds (tc_seg.hpp)
    // chain rounds (tc_chain.hpp): reference rank per group head slot, code per text position, block summaries of the scan
    u32 *chain_ref, *chain_code, *chain_summ;
};

// the MSD round 0 pays from this many suffixes on (level-3 buckets of >= ~64 members on DNA)
static inline u64 msd_min_n() { return (u64)env_int("TC_SA_MSD_MIN_LOG2", 27) >= 40 ? ~0ull : 1ull << env_int("TC_SA_MSD_MIN_LOG2", 27); }
// (and from 1024 suffixes on whatever the variable says: the partition kernels' stand-in addresses -- a quad of the arrays,
// 16 aligned bytes of the text -- must exist; texts of less than a tile are one tile, loaded pair by pair)
static inline bool msd_wanted(u64 N) { return env_int("TC_SA_MSD", 1) != 0 && N >= msd_min_n() && N >= 1024; }

// The tables of the segmented sort (tc_seg.hpp) for N slots, in the order sa_carve has always carved them; the debug entry
// tc_dbg_seg_sort carves the same for its m pairs, so a test runs with the cap_runs / cap_tiles of a text of m suffixes.
static void seg_carve(Arena &A, u64 N, SegBuffers &g) {
    g.cap_runs = (size_t)(N / SEG_CAP + 2);
    g.cap_tiles = (size_t)(N / SEG_PT + 2) + g.cap_runs;
    g.segbits = A.get<u64>(seg_bit_words(N));
    g.ybits = A.get<u64>(seg_bit_words(N));
    for (int q = 0; q < 2; q++) {
        g.lstart[q] = A.get<u32>(g.cap_runs);
        g.lsize[q] = A.get<u32>(g.cap_runs);
        g.ltbase[q] = A.get<u32>(g.cap_runs);
        g.lshift[q] = A.get<u32>(g.cap_runs);
    }
    g.tile_seg = A.get<u32>(g.cap_tiles);
    g.hist = A.get<u32>(g.cap_runs * 256);
    g.mm = A.get<u32>(g.cap_runs * 2);
    g.counters = A.get<u32>(64);
}

static size_t sa_carve(Arena &A, u64 N, SaBuffers &b, bool own_v1) {
    b.k0 = A.get<u64>(N + 32);   // (+ 32: as two arrays of 32-bit halves -- the split layout of MSD level 1 -- each half is rounded up to a 128-byte line)
    b.k1 = A.get<u64>(N);
    b.v0 = A.get<u32>(N);
    b.v1 = own_v1 ? A.get<u32>(N) : nullptr;
    b.isa = A.get<u32>(N + 1);
    b.v2 = A.get<u32>(N);
    b.sparse_cap = N / 8 + 1024;
    for (int s = 0; s < 2; s++) {
        for (int q = 0; q < 3; q++) b.act[s][q] = A.get<u32>(N);
        b.act[s][3] = A.get<u32>(b.sparse_cap);
        b.sk[s] = A.get<u64>(b.sparse_cap);
        b.sv[s] = A.get<u32>(b.sparse_cap);
    }
    b.t_idx = A.get<u32>(b.sparse_cap);
    b.t_rank = A.get<u32>(b.sparse_cap);
    b.t_bits = A.get<u64>(N / 64 + 2);
    b.t_dir = A.get<u32>(N / 64 + 2);
    b.t_bsum = A.get<u32>(N / 64 / BDIR_TILE + 2);
    b.fin_rc = A.get<u32>(FIN_REGIONS * FIN_RSTRIDE + 128);
    b.kdir = A.get<u32>(((size_t)1 << SA_KDIR_BITS) + 2 + ((size_t)1 << SA_KDIR_BITS) / KDF_CHUNK + 64);   // directory + block minima of its fill
    b.hist = A.get<u32>(RDX_MAX_PASSES * RDX_BINS);
    b.rstatus = A.get<u64>(radix_status_words(N));
    b.gstatus = A.get<u64>(2 * (size_t)tc_cdiv(N, GRP_TILE) + 4);
    b.counts = A.get<u32>(260);
    seg_carve(A, N, b.seg);
    for (int l = 0; l <= MSD_LEVELS; l++) b.msd_pstart[l] = b.msd_pcnt[l] = nullptr;
    if (msd_wanted(N)) {
        b.msd_grid = 256 * MSD_BPC;   // fixed for the carve; the launch uses min(this, CUs x workgroups per CU)
        size_t np = 1;
        for (int l = 0; l <= MSD_LEVELS; l++, np *= 256) {
            b.msd_pstart[l] = A.get<u32>(np);
            b.msd_pcnt[l] = A.get<u32>(np);
            if (l < MSD_LEVELS) {
                b.msd_tpre[l] = A.get<u32>(np + 1);
                b.msd_seg[l] = A.get<u32>((np + b.msd_grid) * 256);
            }
        }
        b.msd_joint = A.get<u32>((size_t)256 * 256 * 256);
        b.tp.key = A.get<u64>((size_t)1 << TP_SLOT_BITS);
        b.tp.grp = A.get<u32>((size_t)1 << TP_SLOT_BITS);
        b.tp.cnt = A.get<u32>((size_t)1 << TP_SLOT_BITS);
        b.tp.bloom = A.get<u32>(((size_t)1 << TP_BLOOM_LOG2) / 32);
    }
    // (carved last: everything above keeps the offsets it had before the chain rounds existed)
    b.chain_ref = A.get<u32>(N + 1);
    b.chain_code = A.get<u32>(N + 1);
    b.chain_summ = A.get<u32>(chain_summ_words());
    return A.off;
}

// ---- scalar slots ----------------------------------------------------------------------------------------------
// The words of ctx->d_scalars (device) and ctx->h_scalars (pinned mirror, first 64) the sort uses.  Kernels write some
// of them by number, so the numbers stay.
enum SaSlot {
    SA_SLOT_PRIMARY = 0,      // primary_kernel: the primary index
    SA_SLOT_ACTIVE = 1,       // group_kernel: members of the next active set
    SA_SLOT_PROBE = 11,       // tied_probe_kernel: tied positions found again in the text
    SA_SLOT_TIED = 12,        // round 0: low half tied members, high half flags (1 over-long bucket left to the fix pass,
                              // 2 whole buckets tied, 4 bucket above the finish chunk, 8 joint counts off)
    SA_SLOT_DROPPED = 13,     // finish_filter_kernel: members the fix pass voided
    SA_SLOT_SAMPLE = 14,      // sample_dup_kernel: duplicates among the sample
    SA_SLOT_MAXCHILD = 15,    // msd_scan_kernel of the last level: longest level-3 bucket
    SA_SLOT_SEG = 24,         // (host only) seg_sort_pairs: low half long runs, high half tiles of the level at hand
    SA_SLOT_ERR = 62,         // (host only) the device error word as ticket_check read it
    SA_SLOT_MSD_PROF = 64,    // (device only, MSD_PROFILE) 16 words per MSD level
    SA_SLOT_MSDK_PROF = 112,  // (device only, MSDK_PROFILE) 10 words
    SA_SLOT_MSD_DIR = 122,    // (device only) low half: directory fills of the aligned MSD level, summed over workgroups
};
static inline u32 sa_slot_lo(const tc_ctx *ctx, int slot) { return (u32)(ctx->h_scalars[slot] & 0xffffffffu); }
static inline u32 sa_slot_hi(const tc_ctx *ctx, int slot) { return (u32)(ctx->h_scalars[slot] >> 32); }
// the device slot as two u32 ([0] low half, [1] high half)
static inline u32 *sa_dev_slot(tc_ctx *ctx, int slot) { return reinterpret_cast<u32 *>(ctx->d_scalars + slot); }

#ifdef SEG_PROFILE
static void seg_profile_dump(tc_ctx *ctx, u32 m) {   // cycles per phase of thread 0, per window (diagnostic build only)
    u64 h[16];
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    TC_HIP(ctx, hipMemcpyFromSymbol(h, HIP_SYMBOL(seg_prof), sizeof h));
    const double w = (double)(h[7] | 1);
    fprintf(stderr, "seg_small: %llu members, %llu windows (that sort), mid members per window %.0f | cycles per window: bits %.0f attr+masks %.0f (prefix) %.0f image %.0f tiny+compact %.0f tiny store %.0f network %.0f store %.0f\n",
            (unsigned long long)m, (unsigned long long)h[7], h[8] / w, h[0] / w, h[1] / w, 0.0, h[2] / w, h[3] / w, h[4] / w, h[5] / w, h[6] / w);
    memset(h, 0, sizeof h);
    TC_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(seg_prof), h, sizeof h));
}
#else
static inline void seg_profile_dump(tc_ctx *, u32) {}
#endif

// The sort of one doubling round (tc_seg.hpp): keys (grp << 32 | rank, grp non-decreasing) and values, m members, ranks
// below 2^rbits.  The result is in (kx, vx); (ky, vy) is scratch of the same size.  One host synchronisation per
// partition level that has long runs (none: one, for the count of long runs).  levels (host, 16 words, optional; tests):
// [2L], [2L + 1] = the long runs and tiles read back before level L, zeros after the last.
static void seg_sort_pairs(tc_ctx *ctx, SegBuffers &g, u64 *kx, u32 *vx, u64 *ky, u32 *vy, u32 m, int rbits,
                           u32 *levels = nullptr) {
    hipStream_t s = ctx->stream;
    if (levels) memset(levels, 0, 16 * sizeof(u32));
    const u32 nwords = (u32)seg_bit_words(m);
    TC_HIP(ctx, hipMemsetAsync(g.ybits, 0, (size_t)nwords * sizeof(u64), s));
    TC_HIP(ctx, hipMemsetAsync(g.counters, 0, 8 * sizeof(u32), s));
    u32 igrid = tc_cdiv((u64)nwords * 64, 256);
    if (igrid > 16384) igrid = 16384;
    seg_init_kernel<<<igrid, 256, 0, s>>>(kx, m, g.segbits, nwords, g.lstart[0], g.lsize[0], g.ltbase[0], g.lshift[0],
                                          (u32)(rbits > 8 ? rbits - 8 : 0), g.counters, (u32)g.cap_runs);
    TC_LAUNCH_CHECK(ctx);
    // (a level either splits a run by 8 more rank bits or -- all members in one digit -- re-lists it with a better shift:
    // at most 4 of the first kind and 4 of the second per run)
    const int nlev = 8;
    int cur = 0;
    for (int L = 0;; L++) {
        TC_HIP(ctx, hipMemcpyAsync(&ctx->h_scalars[SA_SLOT_SEG], g.counters + 2 * cur, 2 * sizeof(u32), hipMemcpyDeviceToHost, s));
        TC_HIP(ctx, hipStreamSynchronize(s));
        const u32 S = sa_slot_lo(ctx, SA_SLOT_SEG), T = sa_slot_hi(ctx, SA_SLOT_SEG);
        if (S == 0) break;
        if (levels && L < nlev) { levels[2 * L] = S; levels[2 * L + 1] = T; }
        if (L >= nlev) TC_FAIL(ctx, TC_ERR_INTERNAL, "segmented sort: %u runs still unsorted after %d levels", S, nlev);
        if (S > g.cap_runs || T > g.cap_tiles) TC_FAIL(ctx, TC_ERR_INTERNAL, "segmented sort: %u long runs / %u tiles exceed the tables", S, T);
        const int nxt = cur ^ 1;
        TC_HIP(ctx, hipMemsetAsync(g.hist, 0, (size_t)S * 256 * sizeof(u32), s));
        seg_mm_init_kernel<<<tc_cdiv(S, 256), 256, 0, s>>>(g.mm, S);
        TC_LAUNCH_CHECK(ctx);
        TC_HIP(ctx, hipMemsetAsync(g.counters + 2 * nxt, 0, 2 * sizeof(u32), s));
        u32 wgrid = tc_cdiv(S, 4);
        if (wgrid > 8192) wgrid = 8192;
        seg_tilemap_kernel<<<wgrid, 256, 0, s>>>(g.lsize[cur], g.ltbase[cur], S, g.tile_seg, (u32)g.cap_tiles);
        TC_LAUNCH_CHECK(ctx);
        seg_count_kernel<<<T, 256, 0, s>>>(kx, ky, g.lstart[cur], g.lsize[cur], g.ltbase[cur], g.lshift[cur], g.tile_seg, g.counters + 2 * cur, g.hist, g.mm);
        TC_LAUNCH_CHECK(ctx);
        seg_scan_kernel<<<wgrid, 256, 0, s>>>(g.lstart[cur], g.lsize[cur], g.lshift[cur], g.counters + 2 * cur, g.hist, g.mm, g.segbits, 0,
                                              g.lstart[nxt], g.lsize[nxt], g.ltbase[nxt], g.lshift[nxt], g.counters + 2 * nxt, (u32)g.cap_runs);
        TC_LAUNCH_CHECK(ctx);
        seg_scatter_kernel<<<T, 256, 0, s>>>(kx, vx, ky, vy, g.lstart[cur], g.lsize[cur], g.ltbase[cur], g.lshift[cur], g.tile_seg, g.counters + 2 * cur,
                                             g.hist, g.mm, g.ybits);
        TC_LAUNCH_CHECK(ctx);
        cur = nxt;
    }
    seg_small_kernel<<<tc_cdiv(m, SEG_SPAN), SEG_NT, 0, s>>>(kx, vx, ky, vy, m, g.segbits, g.ybits);
    TC_LAUNCH_CHECK(ctx);
    seg_profile_dump(ctx, m);
}

static void sa_choose_config(const u32 *counts, u64 n, int forced_fields, SaConfig &c) {
    u32 sig = 0;
    double H = 0;
    for (int v = 0; v < 256; v++) {
        c.lut[v] = 0;
        if (counts[v]) {
            c.lut[v] = (u16)(++sig);
            double p = (double)counts[v] / (double)n;
            H -= p * log2(p);
        }
    }
    c.sigma_text = sig;
    c.B = sig + 1;
    if (c.B <= 16) {
        c.w = 8;
        c.s = 1;
        u32 pw = c.B;
        while (pw * c.B <= 256) {
            pw *= c.B;
            c.s++;
        }
    } else {
        c.s = 1;
        c.w = (u32)ceil_log2_u64(c.B);
    }
    u32 pmax = 56 / c.w;  // the low 8 key bits carry the preceding text byte
    // fields so that an iid text of this entropy has ~2^-8 of its suffixes still tied
    double need = (double)ceil_log2_u64(n + 1) + 8.0;
    double per_field = H * c.s;
    u32 P = pmax;
    if (per_field > 1e-9) {
        double pf = ceil(need / per_field);
        if (pf < (double)pmax) P = (u32)pf;
    }
    if (P < 1) P = 1;
    if (forced_fields > 0) P = (u32)forced_fields;
    if (P > pmax) P = pmax;
    c.P = P;
    c.h0 = P * c.s;
    c.entropy = H;
}

// Builds SA (d_sa, N entries), last column (d_L, N bytes) and primary for the
// device text.  d_sa may be null (workspace buffer used).  counts256_out (host,
// optional) receives the byte histogram.
static void sa_run(tc_ctx *ctx, SaBuffers &b, const u8 *d_text, u64 n, u32 *d_sa, u8 *d_L,
                   u64 *primary, u32 *counts256_out);

// The sharded tile tickets of round 0's radix passes (the only passes that draw them) assume blocks
// start in roughly increasing blockIdx order.  If a bounded look-back spin ran out (bit 1 of the error
// word), the scatter of that pass left slots unwritten, and a stale value in them is a suffix start that
// finish_kernel, group_kernel or a later round's ISA scatter would use as an index.  So the flag is read
// right after those passes, before anything consumes their output, and the attempt is abandoned:
// sa_build runs the sort again with the single counter (every status, ticket and histogram word is
// zeroed again where it is used, and SA / last column are written anew, as in any call on a reused
// workspace).  TC_DBG_TICKET_TRIP=1 (tests): the first attempt's check finds the flag set -- only the
// flag is simulated, the passes themselves ran normally.
struct TicketTrip {};
__global__ void err_or_kernel(u32 *err, u32 bits) { atomicOr(err, bits); }
static void ticket_check(tc_ctx *ctx) {
    if (env_int("TC_DBG_TICKET_TRIP", 0) != 0) {
        err_or_kernel<<<1, 1, 0, ctx->stream>>>(ctx->d_err, 2u);
        TC_LAUNCH_CHECK(ctx);
    }
    TC_HIP(ctx, hipMemcpyAsync(&ctx->h_scalars[SA_SLOT_ERR], ctx->d_err, sizeof(u32), hipMemcpyDeviceToHost,
                               ctx->stream));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (sa_slot_lo(ctx, SA_SLOT_ERR) & 2u) throw TicketTrip{};
}

static void sa_build(tc_ctx *ctx, Arena &A, const u8 *d_text, u64 n, u32 *d_sa, u8 *d_L,
                     u64 *primary, u32 *counts256_out, bool dry) {
    const u64 N = n + 1;
    SaBuffers b;
    sa_carve(A, N, b, d_sa == nullptr);
    if (dry) return;
    try {
        sa_run(ctx, b, d_text, n, d_sa, d_L, primary, counts256_out);
    } catch (const TicketTrip &) {
        tc_memset_async(ctx, ctx->d_err, 0, sizeof(u32));
        ctx->safe_tickets = 1;
        ctx->ticket_fallbacks++;
        sa_run(ctx, b, d_text, n, d_sa, d_L, primary, counts256_out);
    }
    ctx->stats.ticket_fallbacks = ctx->ticket_fallbacks;
}

// ---- the state of one sa_run -------------------------------------------------------------------------------------
struct SaRun {
    tc_ctx *ctx;
    SaBuffers &b;
    const u8 *text;   // device text, n bytes
    u64 n, N;         // N = n + 1 suffixes
    int rbits;        // bits of a rank or slot: values < N
    u32 *d_sa;        // the caller's array, or null
    u32 *sa;          // where the suffix array goes: d_sa, or the workspace's v1
    u8 *d_L;          // last column
    SaKnobs K;
    SaConfig cfg;     // (round 0 widens P; the full path sets it again)
    // ranks by regions (tc_sa.hpp, "dense ranks by regions"): sets of at least bin_min members; part_act1: the second
    // active set as N u64 of partition scratch (free whenever the first one is being built)
    int rshift;
    u64 bin_min;
    u64 *part_act1;
    bool part_act1_ok;
    // what round 0 hands to the rest
    u64 m = 0;                     // tied suffixes, in act[0]
    u64 h_start = 0;               // symbols every tied group shares
    const u64 *skeys = nullptr;    // the round-0 keys in final order, or
    const u64 *tkeys = nullptr;    // the keys ordered by their bits >= tkeys_shift only
    int tkeys_shift = 0;
    bool isa_ready = false;        // the full path stored the dense ranks already
    // what sa_rank_tables hands to the doubling rounds
    bool dense = false;
    RankLookup rl = {};
    std::chrono::steady_clock::time_point trace_t0;   // (TC_SA_TRACE) start of the step at hand

    hipStream_t stream() const { return ctx->stream; }
    tc_stats &st() const { return ctx->stats; }
};

// one sa_fill per parameter struct the kernels take: the alphabet configuration, field by field
template <class X>
static inline void sa_fill(const SaConfig &c, X &x) {   // RadixKeyGen, KeyBuildParams, RankLookup
    x.B = c.B; x.w = c.w; x.s = c.s; x.P = c.P;
    memcpy(x.lut, c.lut, sizeof x.lut);
}
static inline void sa_fill(const SaConfig &c, MsdTextDigit &x) {
    x.B = c.B; x.s = c.s;
    memcpy(x.lut, c.lut, sizeof x.lut);
}
// the key generator of the configuration at hand, without the byte hash
static RadixKeyGen sa_keygen(const SaRun &R) {
    RadixKeyGen kg;
    sa_fill(R.cfg, kg);
    kg.n_text = (u32)R.n;
    kg.hash_ok = 0; kg.hsh = 0; kg.tlo = 0; kg.thi = 0;
    return kg;
}
// radix buffers over two key and two value arrays, with the sort's shared histogram and status words
static RadixBuffers sa_radix_buffers(const SaRun &R, u64 *keys, u64 *keys_alt, u32 *vals, u32 *vals_alt) {
    RadixBuffers rb;
    rb.keys = keys; rb.keys_alt = keys_alt; rb.vals = vals; rb.vals_alt = vals_alt;
    rb.hist = R.b.hist; rb.status = R.b.rstatus; rb.status_cap = radix_status_words(R.N);
    return rb;
}
static RadixBuffers sa_sparse_buffers(const SaRun &R) {   // the sparse round buffers
    return sa_radix_buffers(R, R.b.sk[0], R.b.sk[1], R.b.sv[0], R.b.sv[1]);
}

// ---- diagnostics (TC_SA_TRACE, *_PROFILE builds): nothing happens when they are off -----------------------------
static void sa_trace_buffers(const SaRun &R) {
    if (R.K.trace != 2) return;
    fprintf(stderr, "textcomp: buffers text %p k0 %p k1 %p v0 %p v1 %p sa %p L %p\n", (const void *)R.text, (void *)R.b.k0,
            (void *)R.b.k1, (void *)R.b.v0, (void *)R.b.v1, (void *)R.d_sa, (void *)R.d_L);
}
// wall time of the step that ends here, closed by a stream sync -- experiments only
static void sa_trace_step(SaRun &R, const char *what, u64 count) {
    if (!R.K.trace) return;
    (void)hipStreamSynchronize(R.stream());
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "textcomp:   %-28s %10llu  %8.3f ms\n", what, (unsigned long long)count,
            std::chrono::duration<double, std::milli>(t1 - R.trace_t0).count());
    R.trace_t0 = t1;
}
// order-free sums of the tied members' keys, slots and groups after the key-only levels
static void sa_trace_tied_checksums(SaRun &R, u32 fm) {
    if (R.K.trace < 2 || fm == 0) return;
    tc_ctx *ctx = R.ctx;
    std::vector<u32> hk(fm), hh(fm), hs(fm), hg(fm);
    tc_d2h(ctx, hk.data(), R.b.act[0][1], fm * sizeof(u32));
    tc_d2h(ctx, hh.data(), R.b.act[0][3], fm * sizeof(u32));
    tc_d2h(ctx, hs.data(), R.b.act[0][0], fm * sizeof(u32));
    tc_d2h(ctx, hg.data(), R.b.act[0][2], fm * sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(R.stream()));
    u64 a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (u32 i = 0; i < fm; i++) { a1 += hk[i]; a2 += hh[i]; a3 += hs[i]; a4 += hg[i]; }
    fprintf(stderr, "textcomp: tied members: sum klo %llx khi %llx slot %llx grp %llx\n", (unsigned long long)a1, (unsigned long long)a2, (unsigned long long)a3, (unsigned long long)a4);
    for (u32 i = 0; i < fm && i < 6; i++) fprintf(stderr, "textcomp:   member %u: klo %08x khi %06x slot %u grp %u\n", i, hk[i], hh[i], hs[i], hg[i]);
}
// members per group-size class of the active set `cur` (hist is free between two rounds)
static void sa_trace_group_sizes(SaRun &R, int cur, u32 mm) {
    if (!R.K.trace) return;
    tc_ctx *ctx = R.ctx;
    u64 *gh = reinterpret_cast<u64 *>(R.b.hist);
    tc_memset_async(ctx, gh, 0, 32 * sizeof(u64));
    group_size_hist_kernel<<<tc_cdiv(mm, 256), 256, 0, R.stream()>>>(R.b.act[cur][0], R.b.act[cur][2], mm, gh);
    u64 hh32[32];
    tc_d2h(ctx, hh32, gh, sizeof hh32);
    (void)hipStreamSynchronize(R.stream());
    fprintf(stderr, "textcomp:   members by group size 2^c:");
    for (int c = 0; c < 32; c++) if (hh32[c]) fprintf(stderr, " %d:%.1f%%", c, 100.0 * (double)hh32[c] / (double)mm);
    fprintf(stderr, "\n");
    R.trace_t0 = std::chrono::steady_clock::now();
}
// what a chain round's tables hold for the members of the active set `cur`
static void sa_trace_chain_tables(SaRun &R, int cur, u32 mm, u32 hh, const ChainDims &cd, const u64 *chain_path, const u64 *chain_sign) {
    if (!R.K.trace) return;
    tc_ctx *ctx = R.ctx;
    unsigned long long *dg = reinterpret_cast<unsigned long long *>(R.b.hist);
    tc_memset_async(ctx, dg, 0, 8 * sizeof(u64));
    chain_diag_kernel<<<4096, 256, 0, R.stream()>>>(R.b.act[cur][1], R.b.act[cur][2], mm, chain_path, chain_sign, R.b.chain_code, dg);
    u64 hd[8];
    tc_d2h(ctx, hd, dg, sizeof hd);
    (void)hipStreamSynchronize(R.stream());
    fprintf(stderr, "textcomp:   chain tables (h = %u, %u x %u cells of %u rows, %s ranks): members %u, on path %llu, k = 0: %llu, largest k %llu\n",
            hh, cd.nb, cd.h, cd.bk, R.dense ? "dense" : "sparse", mm, (unsigned long long)hd[0], (unsigned long long)hd[1], (unsigned long long)hd[2]);
    R.trace_t0 = std::chrono::steady_clock::now();
}
#ifdef MSDK_PROFILE
static void msdk_profile_dump(tc_ctx *ctx) {
    u64 h[10];
    tc_d2h(ctx, h, ctx->d_scalars + SA_SLOT_MSDK_PROF, sizeof h);
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double c = (double)(h[8] | 1);
    fprintf(stderr, "finish (key-only): chunks %llu, keys per chunk %.0f | cycles per chunk: land %.0f B %.0f zero+B %.0f bins+B %.0f scan+B %.0f scatter+B %.0f walk+prefetch+rank+B %.0f copy-out %.0f\n",
            (unsigned long long)h[8], h[9] / c, h[0] / c, h[1] / c, h[2] / c, h[3] / c, h[4] / c, h[5] / c, h[6] / c, h[7] / c);
    tc_memset_async(ctx, ctx->d_scalars + SA_SLOT_MSDK_PROF, 0, sizeof h);
}
#else
static inline void msdk_profile_dump(tc_ctx *) {}
#endif
#ifdef MSD_PROFILE
static void msd_profile_dump(tc_ctx *ctx) {   // cycles per phase of workgroup 0 / thread 0, per level (diagnostic build only)
    u64 h[48];
    tc_d2h(ctx, h, ctx->d_scalars + SA_SLOT_MSD_PROF, sizeof h);
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int l = 0; l < MSD_LEVELS; l++)
        fprintf(stderr, "msd level %d: tiles %llu | cursor+B0 %llu keygen/S1+B1 %llu S2 %llu S3 %llu land %llu B3 %llu S4 %llu (cycles per tile)\n", l + 1,
                (unsigned long long)h[16 * l + 1], (unsigned long long)(h[16 * l] / (h[16 * l + 1] | 1)), (unsigned long long)(h[16 * l + 2] / (h[16 * l + 1] | 1)),
                (unsigned long long)(h[16 * l + 3] / (h[16 * l + 1] | 1)), (unsigned long long)(h[16 * l + 4] / (h[16 * l + 1] | 1)), (unsigned long long)(h[16 * l + 5] / (h[16 * l + 1] | 1)),
                (unsigned long long)(h[16 * l + 6] / (h[16 * l + 1] | 1)), (unsigned long long)(h[16 * l + 7] / (h[16 * l + 1] | 1)));
    for (int l = 0; l < MSD_LEVELS; l++)
        fprintf(stderr, "   level %d, S1 alone per tile: wave 0 %llu, last wave %llu cycles; slowest wave B0 -> before B1 %llu, B0 -> prefetch issued %llu\n", l + 1,
                (unsigned long long)(h[16 * l + 8] / (h[16 * l + 1] | 1)), (unsigned long long)(h[16 * l + 9] / (h[16 * l + 1] | 1)),
                (unsigned long long)(h[16 * l + 10] / (h[16 * l + 1] | 1)), (unsigned long long)(h[16 * l + 11] / (h[16 * l + 1] | 1)));
    for (int l = 0; l < MSD_LEVELS; l++)
        fprintf(stderr, "   level %d, ends of segments: %llu, %llu cycles each (flush, barriers, next ranges; outside the per-tile stamps)\n", l + 1,
                (unsigned long long)h[16 * l + 13], (unsigned long long)(h[16 * l + 12] / (h[16 * l + 13] | 1)));
    tc_memset_async(ctx, ctx->d_scalars + SA_SLOT_MSD_PROF, 0, sizeof h);
}
#else
static inline void msd_profile_dump(tc_ctx *) {}
#endif

// tc_dbg_msd_dir: whether the last sort's aligned level kept its directory, and the fills the device counted
static void sa_dbg_msd_dir(tc_ctx *ctx, uint32_t out[2]) {
    u64 w = 0;
    out[0] = ctx->msd_dir_used ? 1u : 0u;
    out[1] = 0;
    if (ctx->msd_dir_used) {   // (the word is the last sort's: msd_root_kernel zeroes it)
        tc_d2h(ctx, &w, ctx->d_scalars + SA_SLOT_MSD_DIR, sizeof w);
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        out[1] = (u32)(w & 0xffffffffu);
    }
}

// ---- shared steps ----------------------------------------------------------------------------------------------
// group_kernel over sorted (keys, vals) as `ga` describes them; fills in the text, the outputs and the look-back words.
// Leaves the next active set where ga.out_* point and its size in SA_SLOT_ACTIVE (sa_fetch_m).
static void sa_run_group(SaRun &R, bool init, GroupArgs ga) {
    tc_ctx *ctx = R.ctx;
    hipStream_t s = R.stream();
    const u32 gtiles = tc_cdiv(R.N, GRP_TILE);
    u32 tiles = tc_cdiv(ga.count, GRP_TILE);
    tc_memset_async(ctx, R.b.gstatus, 0, (2 * (size_t)gtiles + 4) * sizeof(u64));
    ga.text = R.text; ga.sa = R.sa; ga.L = R.d_L;
    ga.status_max = R.b.gstatus; ga.status_sum = R.b.gstatus + gtiles;
    ga.ticket = reinterpret_cast<u32 *>(R.b.gstatus + 2 * (size_t)gtiles);
    ga.scalars = ctx->d_scalars; ga.err = ctx->d_err;
    u32 grid = init ? tc_persistent_grid_for(ctx, group_kernel<true>, GRP_NT, 2)
                    : tc_persistent_grid_for(ctx, group_kernel<false>, GRP_NT, 2);
    if (grid > tiles) grid = tiles;
    if (init) group_kernel<true><<<grid, GRP_NT, 0, s>>>(ga);
    else group_kernel<false><<<grid, GRP_NT, 0, s>>>(ga);
    TC_LAUNCH_CHECK(ctx);
}
// the size of the active set the last group_kernel left (one host synchronisation)
static u64 sa_fetch_m(SaRun &R) {
    tc_d2h(R.ctx, R.ctx->h_scalars, R.ctx->d_scalars, 2 * sizeof(u64));
    TC_HIP(R.ctx, hipStreamSynchronize(R.stream()));
    return R.ctx->h_scalars[SA_SLOT_ACTIVE];
}
// dense ranks of a large set go by regions: group_kernel left (start, rank) pairs in `pairs`, these kernels store them
// into isa.  `part`: N free u64 slots.
static void sa_apply_pairs(SaRun &R, const u64 *pairs, u32 count, u64 *part) {
    tc_ctx *ctx = R.ctx;
    hipStream_t s = R.stream();
    u32 *cursor = R.b.hist;
    rank_cursor_kernel<<<1, 256, 0, s>>>(cursor, R.rshift);
    TC_LAUNCH_CHECK(ctx);
    rank_bin_kernel<<<tc_cdiv(count, RBIN_TILE), RBIN_NT, 0, s>>>(pairs, count, R.rshift, cursor, part, R.N);
    TC_LAUNCH_CHECK(ctx);
    rank_scatter_kernel<<<tc_cdiv(R.N, RSCAT_NT * RSCAT_ITEMS), RSCAT_NT, 0, s>>>(part, R.N, R.rshift, cursor, R.b.isa);
    TC_LAUNCH_CHECK(ctx);
}

// Round-0 keys of all N suffixes by R.cfg, their digit histograms and the radix passes of `plan`.  Returns the buffers:
// .keys / .vals hold the result.  The ping-pong is arranged so that the sorted values land in R.sa -- or, when a finish
// pass follows (sa_in_alt_at_end), in the other buffer, so that the finish pass writes R.sa.  Throws TicketTrip.
static RadixBuffers sa_build_keys_and_sort(SaRun &R, const RadixPlan &plan, bool sa_in_alt_at_end) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    const SaConfig &cfg = R.cfg;
    hipStream_t s = R.stream();
    const u32 n = (u32)R.n;
    KeyBuildParams kp;
    sa_fill(cfg, kp);
    kp.plan.npass = plan.npass;
    for (int p = 0; p < plan.npass; p++) {
        kp.plan.shift[p] = plan.shift[p];
        kp.plan.mask[p] = plan.mask[p];
    }
    tc_memset_async(ctx, b.hist, 0, sizeof(u32) * RDX_MAX_PASSES * RDX_BINS);
    // one shared histogram when every pass is exactly one 8-bit field
    bool onehist = cfg.w == 8 && plan.npass < RDX_MAX_PASSES && R.K.kb_onehist != 0;
    for (int p = 0; p < plan.npass; p++)
        if (plan.mask[p] != 255u || plan.shift[p] % 8 != 0) onehist = false;
    const u32 kgrid = tc_cdiv(R.N, SA_TILE);
    // fused first pass: keys are generated inside the first radix pass (no key array
    // written + re-read); needs the shared-histogram configuration
    const bool fuse = onehist && RDX_TILE == SA_TILE && R.K.keygen_fused != 0;
    R.st().keygen_fused = fuse ? 1u : 0u;
    const RadixKeyGen kg = sa_keygen(R);
    if (fuse) {
        u32 ggrid = tc_cdiv(R.N, 256 * 16 * 4);
        if (ggrid > 2048) ggrid = 2048;
        if (cfg.s == 3) ghist_kernel<3><<<ggrid, 256, 0, s>>>(R.text, n, kp, b.hist);
        else ghist_kernel<0><<<ggrid, 256, 0, s>>>(R.text, n, kp, b.hist);
        TC_LAUNCH_CHECK(ctx);
        keyhist_fix_kernel<<<1, 256, 0, s>>>(R.text, n, kp, b.hist);
    } else if (onehist) {
        // unrolled instances for the DNA-like configuration (3 symbols per field)
        if (cfg.s == 3 && cfg.P == 6) keybuild_kernel<true, 3, 6><<<kgrid, SA_NT, 0, s>>>(R.text, n, kp, b.k0, b.hist);
        else if (cfg.s == 3 && cfg.P == 5) keybuild_kernel<true, 3, 5><<<kgrid, SA_NT, 0, s>>>(R.text, n, kp, b.k0, b.hist);
        else keybuild_kernel<true, 0, 0><<<kgrid, SA_NT, 0, s>>>(R.text, n, kp, b.k0, b.hist);
        TC_LAUNCH_CHECK(ctx);
        keyhist_fix_kernel<<<1, 256, 0, s>>>(R.text, n, kp, b.hist);
    } else {
        keybuild_kernel<false, 0, 0><<<kgrid, SA_NT, 0, s>>>(R.text, n, kp, b.k0, b.hist);
    }
    TC_LAUNCH_CHECK(ctx);
    const bool even = plan.npass % 2 == 0;
    const bool start_in_sa = sa_in_alt_at_end ? !even : even;
    RadixBuffers rb = start_in_sa ? sa_radix_buffers(R, b.k0, b.k1, R.sa, b.v0) : sa_radix_buffers(R, b.k0, b.k1, b.v0, R.sa);
    ctx->pev_used = 0;
    const bool xcd_group = !ctx->safe_tickets && R.K.xcd_group != 0;
    radix_sort_pairs(ctx, rb, (u32)R.N, plan, /*gen_idx=*/true, /*hist_ready=*/true, /*timed=*/true,
                     R.text, fuse ? &kg : nullptr, xcd_group);
    if (xcd_group) ticket_check(ctx);   // (throws TicketTrip: nothing below reads a broken scatter)
    return rb;
}

// ---- 1. alphabet -----------------------------------------------------------------------------------------------
// Byte histogram of the text -> R.cfg (and counts256_out).  True: the text is unary and SA, last column and primary
// are already written -- the suffixes are ordered by length, no sort needed (prefix doubling would take log2 n full
// rounds on a zero-filled buffer or "AAAA...").
static bool sa_alphabet(SaRun &R, u32 *counts256_out, u64 *primary) {
    tc_ctx *ctx = R.ctx;
    hipStream_t s = R.stream();
    tc_memset_async(ctx, R.b.counts, 0, 256 * sizeof(u32));
    {
        u32 grid = tc_cdiv(R.n, 256 * 64);
        if (grid > 2048) grid = 2048;
        if (grid < 1) grid = 1;
        hist256_kernel<<<grid, 256, 0, s>>>(R.text, R.n, R.b.counts);
        TC_LAUNCH_CHECK(ctx);
    }
    u32 counts[256];
    tc_d2h(ctx, counts, R.b.counts, sizeof counts);
    TC_HIP(ctx, hipStreamSynchronize(s));
    if (counts256_out) memcpy(counts256_out, counts, sizeof counts);
    sa_choose_config(counts, R.n, R.K.fields, R.cfg);
    if (R.cfg.sigma_text != 1 || R.n == 0) return false;
    unary_sa_kernel<<<tc_cdiv(R.N, 256), 256, 0, s>>>(R.text, (u32)R.n, R.sa, R.d_L);
    TC_LAUNCH_CHECK(ctx);
    *primary = R.n;
    tc_stats &st = R.st();
    st.sigma = 2; st.rounds = 0; st.radix_launches = 0; st.ms_radix = 0;
    return true;
}

// ---- 2. round 0 ------------------------------------------------------------------------------------------------
// Fast path: sort only the top key bits globally (MSD levels, or LSD passes), then a finish kernel orders the (tiny, on
// high-entropy text) equal-prefix buckets by the remaining bits and emits SA / L / the tied set.  Oversize buckets or
// a large tied set => the full path: all P passes, group_kernel<INIT>, dense ISA if needed.

// cheap look before the leap: how many of a sample of suffixes collide on the globally sorted prefix (one host
// synchronisation).  Leaves st.sample_dups.
static void sa_sample(SaRun &R, int topbits) {
    tc_ctx *ctx = R.ctx;
    sample_dup_kernel<<<1, 1024, 0, R.stream()>>>(R.text, (u32)R.n, sa_keygen(R), topbits, sa_dev_slot(ctx, SA_SLOT_SAMPLE));
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[SA_SLOT_SAMPLE], ctx->d_scalars + SA_SLOT_SAMPLE, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(R.stream()));
    R.st().sample_dups = sa_slot_lo(ctx, SA_SLOT_SAMPLE);
}

// What either way of round 0 leaves for sa_round0_collect: SA / last column of the untied suffixes are written, the tied
// set lies in 64 regions of act[1], its size and the flags in the device slot SA_SLOT_TIED.
struct Round0Out {
    bool msd, msd_big, keyonly;
    int tb;                    // key bits that are globally ordered
    FinishArgs fa;             // the tied set's regions and counters (and, LSD, the finish pass's input)
    const u64 *keys;           // the keys, ordered by their top tb bits
    const u64 *keys_sorted;    // MSD: the keys in final order (the big finish wrote them), else null
    int npass;                 // for the statistics
};
// the arguments both finish passes share, for tb globally ordered bits; zeroes the counters they append by
static void sa_round0_begin(SaRun &R, int tb, Round0Out &o) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    const int keybits = (int)(R.cfg.P * R.cfg.w);
    FinishArgs &fa = o.fa;
    o.tb = tb;
    o.keys_sorted = nullptr;
    fa.N = (u32)R.N; fa.tshift = 64 - tb;
    fa.lshift = 64 - keybits; fa.lbits = keybits - tb;
    fa.sa_out = R.sa; fa.L = R.d_L;
    // the lean pass appends to 64 regions of the SECOND active set (one counter each); they are
    // then packed into the first one, which everything below works on
    fa.out_slot = b.act[1][0]; fa.out_idx = b.act[1][1]; fa.out_grp = b.act[1][2];
    fa.act_cap = (u32)R.N; fa.counters = sa_dev_slot(ctx, SA_SLOT_TIED);
    fa.rcount = b.fin_rc; fa.rcap = (u32)(R.N / FIN_REGIONS);
    fa.fix_cap = (u32)(b.sparse_cap - 1024);
    fa.ovbits = b.act[1][0];   // (after the packing) the second active set is unused again
    tc_memset_async(ctx, ctx->d_scalars + SA_SLOT_TIED, 0, 2 * sizeof(u64));
    tc_memset_async(ctx, b.fin_rc, 0, (FIN_REGIONS * FIN_RSTRIDE + 128) * sizeof(u32));
}

// The LSD way: the top pl.topbits key bits by stable passes (keys generated inside the first one where possible), then
// finish_kernel.  Throws TicketTrip.
static Round0Out sa_round0_lsd(SaRun &R, const Round0Plan &pl) {
    Round0Out o;
    o.msd = o.msd_big = o.keyonly = false;
    sa_round0_begin(R, pl.topbits, o);
    R.st().msd_path = 0;
    RadixPlan plan;
    plan.add_range(64 - pl.topbits, 64);
    RadixBuffers rb = sa_build_keys_and_sort(R, plan, /*sa_in_alt_at_end=*/true);
    o.npass = plan.npass;
    o.keys = rb.keys;
    o.fa.keys = rb.keys; o.fa.sa_in = rb.vals;
    const u32 waves = tc_cdiv(R.N, 64 * FIN_WPW);
    finish_kernel<<<tc_cdiv(waves, FIN_NT / 64), FIN_NT, 0, R.stream()>>>(o.fa);
    TC_LAUNCH_CHECK(R.ctx);
    return o;
}

// The MSD way: MSD_LEVELS partition levels by field 0, 1, 2 (keys generated inside the first), then one of the finish
// instances per level-3 parent.  keyonly: the levels move keys without suffix starts (no array was asked for); the tied
// members then leave by slot, group and key (sa_keyonly_recover finds their starts).
static Round0Out sa_round0_msd(SaRun &R, const Round0Plan &pl, bool keyonly) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    const SaConfig &cfg = R.cfg;
    hipStream_t s = R.stream();
    tc_stats &st = R.st();
    const u32 n = (u32)R.n, N = (u32)R.N;
    Round0Out o;
    o.msd = true; o.msd_big = pl.msd_big; o.keyonly = keyonly;
    sa_round0_begin(R, 8 * MSD_LEVELS, o);
    u32 *counters = o.fa.counters;
    RadixKeyGen kg = sa_keygen(R);
    radix_keygen_hash(kg);
    if (R.K.keygen_hash == 0) kg.hash_ok = 0;
    MsdTextDigit td;
    sa_fill(cfg, td);
    td.text = R.text; td.n = n;
    td.hash_ok = kg.hash_ok; td.hsh = kg.hsh; td.tlo = kg.tlo; td.thi = kg.thi;
    u32 G = b.msd_grid < (u32)ctx->num_cus * MSD_BPC ? b.msd_grid : (u32)ctx->num_cus * MSD_BPC;
    if (ctx->reserved_cus > 0 && G > (u32)(ctx->num_cus - ctx->reserved_cus) * MSD_BPC)
        G = (u32)(ctx->num_cus - ctx->reserved_cus) * MSD_BPC;   // (CUs left to the exchange: tc_comm_create)
    if (R.K.msd_grid > 0 && (u32)R.K.msd_grid < G) G = (u32)R.K.msd_grid;
    u32 *maxchild = sa_dev_slot(ctx, SA_SLOT_MAXCHILD);
    msd_root_kernel<<<1, 1, 0, s>>>(b.msd_pstart[0], b.msd_pcnt[0], N, maxchild, sa_dev_slot(ctx, SA_SLOT_MSD_DIR));
    TC_LAUNCH_CHECK(ctx);
    // level 1 writes (k0, v0); level 2 (k1, sa); level 3 (k0, v0); the finish reads (k0, v0)
    // and writes sa / L
    u64 *kbuf[2] = {b.k0, b.k1};
    u32 *vbuf[2] = {keyonly ? nullptr : b.v0, keyonly ? nullptr : R.sa};
    st.msd_keyonly = keyonly ? 1u : 0u;
    ctx->pev_used = 0;
    st.keygen_fused = 1;
    // the last level is "aligned" (one workgroup per parent): its child counts are gathered by the
    // level before it, which saves that level's counting pass over the keys (TC_SA_MSD_JOINT=0: off)
    // (its LDS table has a row per digit made of real symbols only: sigma^s <= 128 of them)
    MsdJointRows jr;
    u32 nrows = 0;
    {
        memset(jr.row, 0xff, sizeof jr.row);
        memset(jr.dig, 0, sizeof jr.dig);
        u32 nd = 1;
        for (u32 j = 0; j < cfg.s; j++) nd *= cfg.B;
        for (u32 d = 0; d < nd && d < 256; d++) {
            bool real = true;
            for (u32 v = d, j = 0; j < cfg.s; j++, v /= cfg.B) real = real && (v % cfg.B) != 0;
            if (real) {
                if (nrows < 128) { jr.row[d] = (u8)nrows; jr.dig[nrows] = (u8)d; }
                nrows++;
            }
        }
    }
    const bool joint = R.K.msd_joint != 0 && nrows <= 128;
    // Split layout (tc_msd.hpp: msd_partition_body; TC_MSD_SPLIT=0: off): key-only levels with the joint count -- level 1
    // leaves the keys as two arrays of 32-bit halves in k0 (khi at its start, klo npad elements on), the joint count reads
    // khi alone, level 2 reads both and writes 64-bit keys as ever.  Everything behind level 2 sees no difference.
    const bool split = keyonly && joint && R.K.msd_split != 0 && MSD_LEVELS == 3;
    u32 *khi = reinterpret_cast<u32 *>(b.k0), *klo = khi + msd_split_npad(N);
    ctx->msd_split_used = split ? 1 : 0;
    // Directory of live parents (tc_msd.hpp: msd_partition_body, DIR; TC_MSD_DIR=0: off): the aligned level only
    const bool dir = joint && R.K.msd_dir != 0;
    ctx->msd_dir_used = dir ? 1 : 0;
    if (joint) tc_memset_async(ctx, b.msd_joint, 0, (size_t)256 * 256 * 256 * sizeof(u32));
    u32 np = 1;
    for (int l = 0; l < MSD_LEVELS; l++, np *= 256) {
        MsdLevel ML;
        ML.pstart = b.msd_pstart[l]; ML.pcnt = b.msd_pcnt[l]; ML.tpre = b.msd_tpre[l];
        ML.nparents = np; ML.shift = 56 - 8 * l; ML.seg = b.msd_seg[l];
        ML.cstart = b.msd_pstart[l + 1]; ML.ccnt = b.msd_pcnt[l + 1];
        ML.aligned = (joint && l == MSD_LEVELS - 1) ? 1 : 0;
        ML.ntot = N; ML.cnt_in = b.msd_joint; ML.flags = counters + 1;
        ML.dbg = ctx->d_scalars + SA_SLOT_MSD_PROF + 16 * l;
        ML.dirfills = sa_dev_slot(ctx, SA_SLOT_MSD_DIR);
        const u64 *kin = l ? kbuf[(l - 1) & 1] : nullptr;
        const u32 *vin = l ? vbuf[(l - 1) & 1] : nullptr;
        msd_prep_kernel<<<1, 1024, 0, s>>>(ML.pcnt, np, b.msd_tpre[l]);
        TC_LAUNCH_CHECK(ctx);
        if (l == 0) msd_count_kernel<true, false><<<G, MSD_NT, 0, s>>>(ML, nullptr, td, nullptr, jr);
        else if (ML.aligned) { /* counts already in msd_joint */ }
        else if (joint && l == MSD_LEVELS - 2 && split) msd_count_hi_kernel<<<G, MSD_NT, 0, s>>>(ML, khi, td, b.msd_joint, jr);
        else if (joint && l == MSD_LEVELS - 2) msd_count_kernel<false, true><<<G, MSD_NT, 0, s>>>(ML, kin, td, b.msd_joint, jr);
        else msd_count_kernel<false, false><<<G, MSD_NT, 0, s>>>(ML, kin, td, nullptr, jr);
        TC_LAUNCH_CHECK(ctx);
        msd_scan_kernel<<<np, 256, 0, s>>>(ML, G, l == MSD_LEVELS - 1 ? maxchild : nullptr);
        TC_LAUNCH_CHECK(ctx);
        const bool ev = ctx->profile && ctx->pev_used < 16;
        if (ev) TC_HIP(ctx, hipEventRecord(ctx->pev[2 * ctx->pev_used], s));
        if (split && l <= 1) {
            if (l == 0) msd_partition_split_kernel<true><<<G, MSD_NT, 0, s>>>(ML, khi, klo, nullptr, R.text, kg);
            else msd_partition_split_kernel<false><<<G, MSD_NT, 0, s>>>(ML, khi, klo, kbuf[1], R.text, kg);
        } else if (dir && ML.aligned) {
            if (keyonly) msd_partition_dir_kernel<false><<<G, MSD_NT, 0, s>>>(ML, kin, nullptr, kbuf[l & 1], nullptr, kg);
            else msd_partition_dir_kernel<true><<<G, MSD_NT, 0, s>>>(ML, kin, vin, kbuf[l & 1], vbuf[l & 1], kg);
        } else if (keyonly) {
            if (l == 0) msd_partition_kernel<true, false><<<G, MSD_NT, 0, s>>>(ML, nullptr, nullptr, kbuf[0], nullptr, R.text, kg);
            else msd_partition_kernel<false, false><<<G, MSD_NT, 0, s>>>(ML, kin, nullptr, kbuf[l & 1], nullptr, R.text, kg);
        } else if (l == 0) msd_partition_kernel<true><<<G, MSD_NT, 0, s>>>(ML, nullptr, nullptr, kbuf[0], vbuf[0], R.text, kg);
        else msd_partition_kernel<false><<<G, MSD_NT, 0, s>>>(ML, kin, vin, kbuf[l & 1], vbuf[l & 1], R.text, kg);
        TC_LAUNCH_CHECK(ctx);
        if (ev) {
            TC_HIP(ctx, hipEventRecord(ctx->pev[2 * ctx->pev_used + 1], s));
            ctx->pev_used++;
        }
    }
    o.keys = kbuf[(MSD_LEVELS - 1) & 1];
    MsdFinishArgs mf;
    mf.keys = o.keys; mf.vals = vbuf[(MSD_LEVELS - 1) & 1];
    mf.pcnt = b.msd_pcnt[MSD_LEVELS - 1];
    mf.cstart = b.msd_pstart[MSD_LEVELS]; mf.ccnt = b.msd_pcnt[MSD_LEVELS];
    mf.sa_out = R.sa; mf.L = R.d_L;
    mf.out_slot = o.fa.out_slot; mf.out_idx = o.fa.out_idx; mf.out_grp = o.fa.out_grp;
    mf.rcount = o.fa.rcount; mf.rcap = o.fa.rcap; mf.counters = counters;
    mf.kout = kbuf[MSD_LEVELS & 1];   // (the key buffer the last level did not write)
    o.keys_sorted = mf.kout;
    mf.whole_list = b.msd_seg[MSD_LEVELS - 1];
    mf.whole_cap = 1u << 20;
    mf.out_khi = b.v0;   // (region layout as out_idx)
    // (equal-mass bins from the level-1 digit counts: tc_msd.hpp; TC_MSD_FINISH_LUT=0: the generic instances bin by key bits)
    MsdFinishLut *flut = reinterpret_cast<MsdFinishLut *>(b.msd_seg[MSD_LEVELS - 1] + 2 * (size_t)mf.whole_cap);
    msd_finish_lut_kernel<<<1, 256, 0, s>>>(b.msd_pcnt[1], flut);
    TC_LAUNCH_CHECK(ctx);
    mf.lut = R.K.msd_finish_lut != 0 ? flut : nullptr;
    if (pl.msd_big && keyonly) {
        msd_finish_kernel<MSDF_BIG_NT, MSDF_BIG_ITEMS, 1, 5, true, false><<<np / 256, MSDF_BIG_NT, 0, s>>>(mf);
        // (no msd_whole_kernel: listed buckets raise bit 1 of the flags, which ends the key-only attempt)
    } else if (pl.msd_big) {
        msd_finish_kernel<MSDF_BIG_NT, MSDF_BIG_ITEMS, 1, 5, true><<<np / 256, MSDF_BIG_NT, 0, s>>>(mf);
        TC_LAUNCH_CHECK(ctx);
        msd_whole_kernel<<<1024, MSDW_NT, 0, s>>>(mf);
    } else if (keyonly && R.K.msd_finish_ko != 0) {
        msd_finish_ko_kernel<3><<<np / 256, 256, 0, s>>>(mf, flut);
        msdk_profile_dump(ctx);
    } else if (keyonly) {
        msd_finish_kernel<MSDF_KO_NT, MSDF_CAP_SMALL / MSDF_KO_NT, 4, 1, false, false><<<np / 256, MSDF_KO_NT, 0, s>>>(mf);
    } else {
        msd_finish_kernel<256, 8, 4, 1, false><<<np / 256, 256, 0, s>>>(mf);
    }
    TC_LAUNCH_CHECK(ctx);
    o.npass = MSD_LEVELS;
    st.msd_path = 1;
    msd_profile_dump(ctx);
    return o;
}

// Key-only levels: the fm tied members in act[0] are known by slot, group and key; finds their suffix starts again by one
// pass over the text (tied_table_kernel, tied_probe_kernel or tied_probe_w_kernel: tc_sa.hpp) and leaves them in act[0][1].  False: more ties
// than the table is made for, whole buckets, or a pass that did not find exactly fm positions.
static bool sa_keyonly_recover(SaRun &R, u32 fm, u32 flags) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    const SaConfig &cfg = R.cfg;
    hipStream_t s = R.stream();
    const u32 n = (u32)R.n;
    bool ok = fm <= TP_MAX_TIED && (u64)fm + 1024 <= b.sparse_cap && !(flags & 2u);
    if (ok) sa_trace_tied_checksums(R, fm);
    if (ok && fm > 0) {
        tc_memset_async(ctx, b.tp.key, 0, sizeof(u64) << TP_SLOT_BITS);
        tc_memset_async(ctx, b.tp.cnt, 0, sizeof(u32) << TP_SLOT_BITS);
        tc_memset_async(ctx, b.tp.bloom, 0, ((size_t)1 << TP_BLOOM_LOG2) / 8);
        u32 *d_total = sa_dev_slot(ctx, SA_SLOT_PROBE);
        tc_memset_async(ctx, d_total, 0, sizeof(u64));
        tied_table_kernel<<<tc_cdiv(fm, 256), 256, 0, s>>>(b.act[0][1], b.act[0][3], b.act[0][2], fm, cfg.B, cfg.s, cfg.P, b.tp);
        TC_LAUNCH_CHECK(ctx);
        RadixKeyGen kgp = sa_keygen(R);
        radix_keygen_hash(kgp);
        // codes from the register table where the alphabet has one (tied_probe_w_kernel), else through the byte image
        const bool wide = kgp.hash_ok != 0 && R.K.keygen_hash != 0 && cfg.B <= 8 && R.K.tied_probe != 0;
        u32 pgrid = (u32)ctx->num_cus * 3;
        if (pgrid > tc_cdiv(n, TPK_TILE)) pgrid = tc_cdiv(n, TPK_TILE);
        switch (cfg.s) {   // (symbols per field: B^s <= 256)
#define TC_PROBE(S) case S: \
            if (wide) tied_probe_w_kernel<S><<<pgrid, TPK_NT, 0, s>>>(R.text, n, kgp, b.tp, b.act[0][0], b.act[0][1], b.act[0][2], d_total, fm); \
            else tied_probe_kernel<S><<<pgrid, TPK_NT, 0, s>>>(R.text, n, kgp, b.tp, b.act[0][0], b.act[0][1], b.act[0][2], d_total, fm); \
            break;
            TC_PROBE(1) TC_PROBE(2) TC_PROBE(3) TC_PROBE(4) TC_PROBE(5) TC_PROBE(6) TC_PROBE(7) TC_PROBE(8)
#undef TC_PROBE
            default: TC_FAIL(ctx, TC_ERR_INTERNAL, "key-only levels: %u symbols per field", cfg.s);
        }
        TC_LAUNCH_CHECK(ctx);
        tc_d2h(ctx, &ctx->h_scalars[SA_SLOT_PROBE], ctx->d_scalars + SA_SLOT_PROBE, sizeof(u64));
        TC_HIP(ctx, hipStreamSynchronize(s));
        ctx->tied_probe_used = wide ? 2 : 1;
        ctx->tied_probe_found = sa_slot_lo(ctx, SA_SLOT_PROBE);
        ok = ctx->tied_probe_found == fm;
    }
    if (R.K.trace)
        fprintf(stderr, "textcomp: key-only levels: %u tied suffixes %s (the pass over the text met %u)\n", fm,
                ok ? "found again in the text" : "-- NOT recoverable: the levels run again with suffix starts", sa_slot_lo(ctx, SA_SLOT_PROBE));
    return ok;
}

// LSD, some buckets are longer than a wave window: the second pass turns them into tied groups (the sorted keys are still
// in place) and voids what the first pass emitted for their members.  Reads the fm members in act[0]; one host
// synchronisation; leaves the new count, flags and the number of voided members.
static void sa_tier2_fix(SaRun &R, const FinishArgs &fa, u32 &fm, u32 &flags, u32 &fm_dropped) {
    tc_ctx *ctx = R.ctx;
    hipStream_t s = R.stream();
    const u32 fm_lean = fm;
    u32 *flagword = sa_dev_slot(ctx, SA_SLOT_TIED) + 1;
    u32 *ndropped = sa_dev_slot(ctx, SA_SLOT_DROPPED);
    tc_memset_async(ctx, flagword, 0, sizeof(u32));
    tc_memset_async(ctx, ndropped, 0, sizeof(u64));
    tc_memset_async(ctx, fa.ovbits, 0, ((size_t)tc_cdiv(R.N, 64) + 1) * sizeof(u64));
    const u32 fwaves = tc_cdiv(R.N, 64 * FIX_WIN);
    finish_fix_kernel<<<tc_cdiv(fwaves, FIN_NT / 64), FIN_NT, 0, s>>>(fa);
    TC_LAUNCH_CHECK(ctx);
    if (fm_lean) {
        finish_filter_kernel<<<tc_cdiv(fm_lean, 256) < 4096u ? tc_cdiv(fm_lean, 256) : 4096u, 256, 0, s>>>(fa.out_slot, fm_lean, fa.ovbits, ndropped);
        TC_LAUNCH_CHECK(ctx);
    }
    tc_d2h(ctx, &ctx->h_scalars[SA_SLOT_TIED], ctx->d_scalars + SA_SLOT_TIED, 2 * sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    fm = sa_slot_lo(ctx, SA_SLOT_TIED);
    flags = sa_slot_hi(ctx, SA_SLOT_TIED);
    fm_dropped = sa_slot_lo(ctx, SA_SLOT_DROPPED);
}

// Brings the fm entries of the tied set in act[0] into SA order (refine relies on it); void entries go last.
static void sa_order_tied(SaRun &R, u32 fm, u32 slot_bits) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    if (fm <= SEG_W && R.K.tiny != 0) {   // (a few thousand members: one workgroup, tc_seg.hpp)
        tied_small_kernel<0><<<1, SEG_NT, 0, s>>>(b.act[0][0], b.act[0][1], b.act[0][2], fm, nullptr, nullptr, nullptr);
        TC_LAUNCH_CHECK(ctx);
        return;
    }
    pack_active_kernel<<<tc_cdiv(fm, 256), 256, 0, s>>>(b.act[0][0], b.act[0][2], fm, b.sk[0]);
    TC_LAUNCH_CHECK(ctx);
    TC_HIP(ctx, hipMemcpyAsync(b.sv[0], b.act[0][1], fm * sizeof(u32), hipMemcpyDeviceToDevice, s));
    RadixPlan ps;
    ps.add_range(32, 32 + (int)slot_bits);
    RadixBuffers rs = sa_sparse_buffers(R);
    radix_sort_pairs(ctx, rs, fm, ps, false, false);
    unpack_active_kernel<<<tc_cdiv(fm, 256), 256, 0, s>>>(rs.keys, fm, b.act[0][0], b.act[0][2]);
    TC_LAUNCH_CHECK(ctx);
    TC_HIP(ctx, hipMemcpyAsync(b.act[0][1], rs.vals, fm * sizeof(u32), hipMemcpyDeviceToDevice, s));
}

// The key round (tc_sa.hpp): the big finish emitted whole buckets as groups that share 9 symbols; the key holds 12 more.
// Orders the R.m members of act[0] by the key's remaining 32 bits (kall: the keys in final order, rewritten in place)
// and regroups them: one round entry more, R.m the members still tied, R.h_start the whole key.  One host sync.
static void sa_key_round(SaRun &R, u64 *kall) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    tc_stats &st = R.st();
    const u32 mm = (u32)R.m;
    key_round_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(b.act[0][0], b.act[0][2], kall, mm, b.sk[0], b.sv[0]);
    TC_LAUNCH_CHECK(ctx);
    seg_sort_pairs(ctx, b.seg, b.sk[0], b.sv[0], b.sk[1], b.sv[1], mm, 32);
    key_round_store_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(b.sk[0], b.act[0][0], mm, kall);
    TC_LAUNCH_CHECK(ctx);
    GroupArgs gk = {};
    gk.keys = b.sk[0]; gk.count = mm; gk.vals = b.sv[0]; gk.vals_are_idx = 0; gk.norank = 1;
    gk.in_slot = b.act[0][0]; gk.in_idx = b.act[0][1];
    gk.out_slot = b.act[1][0]; gk.out_idx = b.act[1][1]; gk.out_grp = b.act[1][2];
    sa_run_group(R, false, gk);
    const u64 m2 = sa_fetch_m(R);
    for (int q = 0; q < 3; q++)
        if (m2) TC_HIP(ctx, hipMemcpyAsync(b.act[0][q], b.act[1][q], m2 * sizeof(u32), hipMemcpyDeviceToDevice, s));
    st.m[st.rounds] = R.m; st.key_bytes[st.rounds] = 8; st.passes[st.rounds] = 1; st.h[st.rounds] = (u32)R.h_start;
    st.rounds++;
    st.seg_rounds++;
    if (R.K.trace)
        fprintf(stderr, "textcomp: key round: %u members of whole buckets ordered by the key's remaining 32 bits, %llu stay tied\n", mm, (unsigned long long)m2);
    R.m = m2;
    R.h_start = R.cfg.h0;   // every tie now shares the whole key
}

enum Round0Result {
    R0_ACCEPTED,      // R.m tied suffixes in act[0], in SA order; R.h_start, R.skeys / R.tkeys set
    R0_GIVE_WAY,      // MSD: the LSD way has to do it.  LSD: the full path
    R0_NEED_STARTS,   // key-only MSD levels: the tied members were not recoverable, the levels run again with suffix starts
};
// Takes what a way of round 0 left (Round0Out): packs the regions of the tied set into act[0], reads its size and the
// flags (one host synchronisation), recovers suffix starts after key-only levels, runs the tier-2 fix pass (LSD), and
// -- accepted -- orders the tied set, runs the key round where whole buckets call for it, and fills the first round's
// statistics.  many_ties is raised when the LSD finish drowned in ties (the full path will want dense ranks).
static Round0Result sa_round0_collect(SaRun &R, Round0Out &o, bool keyround, bool &many_ties) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    tc_stats &st = R.st();
    FinishArgs &fa = o.fa;
    u32 *roff = b.fin_rc + FIN_REGIONS * FIN_RSTRIDE;
    finish_regions_kernel<<<1, 64, 0, s>>>(fa.rcount, fa.rcap, roff, fa.counters);
    TC_LAUNCH_CHECK(ctx);
    if (o.msd && o.keyonly)
        finish_compact_kernel<<<1024, 256, 0, s>>>(roff, fa.rcap, b.act[1][0], b.act[1][1], b.act[1][2],
                                                  b.act[0][0], b.act[0][1], b.act[0][2], b.v0, b.act[0][3], (u32)b.sparse_cap);
    else
        finish_compact_kernel<<<1024, 256, 0, s>>>(roff, fa.rcap, b.act[1][0], b.act[1][1], b.act[1][2],
                                                  b.act[0][0], b.act[0][1], b.act[0][2]);
    TC_LAUNCH_CHECK(ctx);
    fa.out_slot = b.act[0][0]; fa.out_idx = b.act[0][1]; fa.out_grp = b.act[0][2];
    tc_d2h(ctx, &ctx->h_scalars[SA_SLOT_TIED], ctx->d_scalars + SA_SLOT_TIED, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    u32 fm = sa_slot_lo(ctx, SA_SLOT_TIED), over = sa_slot_hi(ctx, SA_SLOT_TIED);
    if (R.K.trace)
        fprintf(stderr, "textcomp: round 0 %s way%s: tied %u, flags 0x%x (1 over-long bucket left to the fix pass, 2 whole buckets tied, 4 bucket above the finish chunk, 8 joint counts off)\n",
                o.msd ? "MSD" : "LSD", o.msd && o.msd_big ? " (big finish)" : "", fm, over);
    if (o.msd && (over & (4u | 8u))) return R0_GIVE_WAY;   // a level-3 bucket beyond the finish chunk (or counts that overflowed)
    if (o.msd && o.keyonly && !sa_keyonly_recover(R, fm, over)) return R0_NEED_STARTS;
    u32 slot_bits = (u32)R.rbits, fm_dropped = 0;
    if (!o.msd && (over & 1u) && fm <= fa.fix_cap && R.K.tier2 != 0) {
        sa_tier2_fix(R, fa, fm, over, fm_dropped);
        slot_bits = (u32)R.rbits + 1;   // the void slot value must sort behind slot N - 1
    }
    // (MSD: rank lookups of untied suffixes count inside an UNSORTED level-3 bucket, ~550 keys
    // each: fine for the few ties of an iid text, hopeless for millions -- the LSD way then)
    if (o.msd && !o.msd_big && fm > (1u << 18)) return R0_GIVE_WAY;
    if ((over & 1u) || fm > b.sparse_cap - 1024) {
        if (!o.msd && fm > b.sparse_cap - 1024) many_ties = true;
        return R0_GIVE_WAY;
    }
    R.m = fm - fm_dropped;
    // whole buckets were emitted as tied groups: they share only the globally sorted
    // symbols, so the doubling starts from those
    if (over & 2u) R.h_start = (u64)(o.tb / (int)R.cfg.w) * R.cfg.s;
    if (o.msd && o.msd_big) {   // keys in final order: ranks of untied suffixes by binary search
        R.skeys = o.keys_sorted;
    } else {
        R.tkeys = o.keys;
        R.tkeys_shift = 64 - o.tb;
    }
    st.finish_pass = 1;
    st.rounds = 1;
    st.m[0] = R.N; st.key_bytes[0] = 8; st.passes[0] = (u32)o.npass; st.h[0] = 0;
    if (R.m > 0) sa_order_tied(R, fm, slot_bits);
    if (o.msd && o.msd_big && (over & 2u) && keyround && R.m >= (u64)R.K.seg_min && R.K.seg != 0)
        sa_key_round(R, const_cast<u64 *>(o.keys_sorted));
    return R0_ACCEPTED;
}

// Round 0 by the fast path.  Reads R.cfg; widens cfg.P.  True: accepted (what sa_round0_collect leaves).  False: the full
// path has to do it, R.cfg.P is whatever was tried, and hopeless / many_ties say whether many ties are to be expected.
static bool sa_round0(SaRun &R, bool &hopeless, bool &many_ties) {
    SaConfig &cfg = R.cfg;
    Round0In in;
    in.entropy = cfg.entropy; in.w = cfg.w; in.s = cfg.s; in.P = cfg.P;
    in.N = R.N;
    in.msd_carved = R.b.msd_pstart[0] != nullptr && msd_wanted(R.N);
    in.want_sa = R.d_sa != nullptr;
    in.sample_dups = 0;
    in.msd_levels = MSD_LEVELS; in.cap_small = MSDF_CAP_SMALL; in.cap_big = MSDF_CAP_BIG;
    in.samp_n = SAMP_N; in.tied_max = TP_MAX_TIED;
    Round0Plan pl;
    sa_round0_depth(in, R.K, pl);
    const bool finish_fits = (int)(cfg.P * cfg.w) - pl.topbits <= 32;   // the finish pass ranks by at most 32 remaining bits
    // if a sample of suffixes already collides heavily on the globally sorted prefix, the tied set would exceed the
    // sparse capacity anyway
    if (finish_fits && R.n >= (1u << 20) && R.K.sample != 0) {
        sa_sample(R, pl.topbits);
        hopeless = R.st().sample_dups > SAMP_N / 10;
    }
    if (!finish_fits || hopeless) return false;
    in.sample_dups = R.st().sample_dups;
    sa_round0_plan(in, R.K, pl);
    if (pl.P != cfg.P) {
        cfg.P = pl.P;
        cfg.h0 = cfg.P * cfg.s;
        R.h_start = cfg.h0;
    }
    // Both ways hand over SA / last column for the untied suffixes and the tied set in act[1] (64 regions).  A text whose
    // level-3 buckets are too long for the MSD finish falls through to the LSD way.
    Round0Result res = R0_GIVE_WAY;
    if (pl.try_msd) {
        Round0Out o = sa_round0_msd(R, pl, pl.keyonly);
        res = sa_round0_collect(R, o, pl.keyround, many_ties);
        if (res == R0_NEED_STARTS) {
            o = sa_round0_msd(R, pl, /*keyonly=*/false);
            res = sa_round0_collect(R, o, pl.keyround, many_ties);
        }
    }
    if (res == R0_GIVE_WAY) {
        R.ctx->msd_split_used = 0;
        R.ctx->msd_dir_used = 0;
        Round0Out o = sa_round0_lsd(R, pl);
        res = sa_round0_collect(R, o, pl.keyround, many_ties);
    }
    return res == R0_ACCEPTED;
}

// Round 0 by the full path: every field is a pass, then group_kernel<INIT> makes the groups of all N suffixes -- with
// the dense ranks in the same pass when many ties are expected.  P_full: the fields sa_choose_config chose.  Leaves R.m,
// R.skeys, R.h_start, R.isa_ready and the first round's statistics.  One host synchronisation.  Throws TicketTrip.
static void sa_full_path(SaRun &R, u32 P_full, bool hopeless, bool many_ties) {
    SaBuffers &b = R.b;
    SaConfig &cfg = R.cfg;
    tc_stats &st = R.st();
    cfg.P = P_full;
    // the sample (or a finish pass that drowned in ties) says the entropy estimate behind P_full does
    // not hold -- natural language, runs: take every field the key has room for; one more pass of
    // the first sort, but the doubling starts deeper and usually saves a round (Zipf text, 256 MiB:
    // 84.6 -> 76.0 ms, five rounds -> four)
    if ((hopeless || st.finish_pass == 0) && R.K.fields == 0 && R.K.deep != 0 && R.K.finish != 0)
        cfg.P = 56 / cfg.w;
    cfg.h0 = cfg.P * cfg.s;
    R.h_start = cfg.h0;
    RadixPlan plan;
    plan.add_range(64 - (int)(cfg.P * cfg.w), 64);
    RadixBuffers rb = sa_build_keys_and_sort(R, plan, /*sa_in_alt_at_end=*/false);
    R.skeys = rb.keys;
    GroupArgs g0 = {};
    g0.keys = R.skeys; g0.count = (u32)R.N; g0.vals = R.sa;
    g0.out_slot = b.act[0][0]; g0.out_idx = b.act[0][1]; g0.out_grp = b.act[0][2]; g0.out_tpos = b.act[0][3];
    // many ties expected (the sample, or a finish pass that just met them -- a text of a period longer than the sample sees:
    // one group pass less, 11 ms per GiB): ranks in the same pass
    const bool ties = hopeless || many_ties;
    if (ties) { g0.isa = b.isa; R.isa_ready = true; }
    const bool g0_pairs = ties && R.N >= R.bin_min && R.part_act1_ok;
    if (g0_pairs) g0.pairs = rb.keys_alt;
    sa_run_group(R, true, g0);
    if (g0_pairs) sa_apply_pairs(R, rb.keys_alt, (u32)R.N, R.part_act1);
    R.m = sa_fetch_m(R);
    st.rounds = 1;
    st.m[0] = R.N; st.key_bytes[0] = 8; st.passes[0] = (u32)plan.npass; st.h[0] = 0;
}

// ---- 3. ranks --------------------------------------------------------------------------------------------------
// Large tied sets: a bitmap of the tied positions + popcount directory instead of a binary search per lookup, and a
// directory into the sorted keys for the ranks of untied suffixes.  t_bits is already filled (table_build_kernel).
static void sa_rank_accel(SaRun &R) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    RankLookup &rl = R.rl;
    const u64 N = R.N;
    const u32 nwords = (u32)(N / 64 + 1);
    const u32 nb = tc_cdiv(nwords, BDIR_TILE);
    bitdir_sum_kernel<<<nb, 256, 0, s>>>(b.t_bits, nwords, b.t_bsum);
    TC_LAUNCH_CHECK(ctx);
    bitdir_spine_kernel<<<1, 1024, 0, s>>>(b.t_bsum, nb);
    TC_LAUNCH_CHECK(ctx);
    bitdir_down_kernel<<<nb, 256, 0, s>>>(b.t_bits, nwords, b.t_bsum, b.t_dir);
    TC_LAUNCH_CHECK(ctx);
    rl.t_bits = b.t_bits; rl.t_dir = b.t_dir;
    const u64 *dkeys = R.tkeys ? R.tkeys : ((R.skeys == b.k0 || R.skeys == b.k1) ? R.skeys : nullptr);   // (sorted keys: a directory serves them too)
    if (!dkeys) return;
    int kb = R.tkeys ? (64 - R.tkeys_shift < SA_KDIR_BITS ? 64 - R.tkeys_shift : SA_KDIR_BITS) : SA_KDIR_BITS;
    // (a directory fine enough to leave ~16 keys per entry: more bits than log2 N - 4 only make it sparser)
    while (kb > 16 && (1ull << kb) > N / 16) kb--;
    if (R.K.kdir_search != 0) {
        kdir_build_kernel<<<tc_cdiv((1ull << kb) + 1, 256), 256, 0, s>>>(dkeys, (u32)N, kb, b.kdir);
        TC_LAUNCH_CHECK(ctx);
    } else {
        const u64 entries = (1ull << kb) + 1;
        const u32 nbk = tc_cdiv(entries, KDF_CHUNK);
        u32 *bmin = b.kdir + ((size_t)1 << SA_KDIR_BITS) + 2;
        tc_memset_async(ctx, b.kdir, 0xff, entries * sizeof(u32));
        kdir_mark_kernel<<<tc_cdiv(N, 256), 256, 0, s>>>(dkeys, (u32)N, kb, b.kdir);
        TC_LAUNCH_CHECK(ctx);
        kdir_fill_min_kernel<<<nbk, 256, 0, s>>>(b.kdir, entries, bmin);
        TC_LAUNCH_CHECK(ctx);
        kdir_fill_spine_kernel<<<1, 1024, 0, s>>>(bmin, nbk);
        TC_LAUNCH_CHECK(ctx);
        kdir_fill_apply_kernel<<<nbk, 256, 0, s>>>(b.kdir, entries, bmin);
        TC_LAUNCH_CHECK(ctx);
    }
    rl.kdir = b.kdir; rl.kdir_bits = kb;
}

// Ranks for the doubling rounds: the dense ISA when many suffixes are tied, else a sparse table of the tied positions + a
// search for everything else (sorted round-0 keys, or the SA itself).  Reads what round 0 left; leaves R.dense and R.rl.
static void sa_rank_tables(SaRun &R) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    RankLookup &rl = R.rl;
    const u64 m = R.m, N = R.N;
    R.dense = m > b.sparse_cap - 1024 || R.K.dense != 0;
    sa_fill(R.cfg, rl);
    rl.text = R.text; rl.n = (u32)R.n; rl.N = (u32)N; rl.h0 = R.cfg.h0;
    if (R.dense && !R.skeys) TC_FAIL(ctx, TC_ERR_INTERNAL, "dense mode needs the sorted keys");
    if (R.dense) {
        if (!R.isa_ready) {  // (also with m == 0: the primary index is read from the ranks)
            GroupArgs gi = {};
            gi.keys = R.skeys; gi.count = (u32)N; gi.vals = R.sa;
            gi.isa = b.isa; gi.isa_only = 1;
            // (scratch: whichever round-0 key buffer does not hold the sorted keys; the second active set)
            u64 *kfree = R.skeys == b.k0 ? b.k1 : b.k0;
            const bool gi_pairs = N >= R.bin_min && R.part_act1_ok && (R.skeys == b.k0 || R.skeys == b.k1);
            if (gi_pairs) gi.pairs = kfree;
            sa_run_group(R, true, gi);
            if (gi_pairs) sa_apply_pairs(R, kfree, (u32)N, R.part_act1);
        }
        rl.isa = b.isa;
        return;
    }
    rl.skeys = R.skeys; rl.tkeys = R.tkeys; rl.tshift = R.tkeys_shift; rl.sa = R.sa; rl.t_idx = b.t_idx; rl.t_rank = b.t_rank; rl.t_n = (u32)m;
    if (m == 0) return;
    const u32 mm = (u32)m;
    if (m <= SEG_W && R.K.tiny != 0) {
        tied_small_kernel<1><<<1, SEG_NT, 0, s>>>(b.act[0][0], b.act[0][1], b.act[0][2], mm, b.t_idx, b.t_rank, b.act[0][3]);
        TC_LAUNCH_CHECK(ctx);
        return;
    }
    widen_u32_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(b.act[0][1], b.sk[0], mm);
    TC_LAUNCH_CHECK(ctx);
    RadixPlan pt;
    pt.add_range(0, R.rbits);
    RadixBuffers rt = sa_sparse_buffers(R);
    radix_sort_pairs(ctx, rt, mm, pt, true, false);
    const bool accel = m >= (u64)R.K.accel_min;
    if (accel) tc_memset_async(ctx, b.t_bits, 0, (size_t)(u32)(N / 64 + 1) * sizeof(u64));
    table_build_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(rt.keys, rt.vals, b.act[0][2], mm,
                                                       b.t_idx, b.t_rank, b.act[0][3],
                                                       accel ? b.t_bits : nullptr);
    TC_LAUNCH_CHECK(ctx);
    if (accel) sa_rank_accel(R);
}

// ---- 4. prefix doubling on the tied suffixes -------------------------------------------------------------------
// One chain round's tables for the mm members of the active set `cur` at depth hh: reference ranks, on-path / sign bits
// of every tied position, their scan along stride hh -> a code per text position in chain_code.  The two bitmaps are
// copied into the reference table's memory once the flags are made, so that they survive the sort of pass 1: pass 2
// asks again which members were on path.
static void sa_chain_codes(SaRun &R, int cur, u32 mm, u32 hh, u64 *chain_path, u64 *chain_sign, u32 chain_words) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    const u64 N = R.N;
    const ChainDims cd = chain_dims(N, hh);
    u64 *pathbits = b.seg.segbits, *signbits = b.seg.ybits;
    u32 *any = b.chain_summ + chain_any_offset();
    tc_memset_async(ctx, b.chain_ref, 0xff, (size_t)N * sizeof(u32));
    chain_ref_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(b.act[cur][0], b.act[cur][1], b.act[cur][2], R.rl, mm, hh, b.chain_ref);
    TC_LAUNCH_CHECK(ctx);
    if (R.dense) {
        u32 fgrid = tc_cdiv(chain_words, 4);
        if (fgrid > 16384) fgrid = 16384;
        chain_flags_kernel<<<fgrid, 256, 0, s>>>(b.isa, b.chain_ref, (u32)N, hh, pathbits, signbits, chain_words);
    } else {
        tc_memset_async(ctx, pathbits, 0, (size_t)chain_words * sizeof(u64));
        tc_memset_async(ctx, signbits, 0, (size_t)chain_words * sizeof(u64));
        u32 fgrid = tc_cdiv(mm, 256);
        if (fgrid > 16384) fgrid = 16384;
        chain_flags_members_kernel<<<fgrid, 256, 0, s>>>(b.act[cur][1], b.act[cur][2], R.rl, mm, hh, b.chain_ref, pathbits, signbits);
    }
    TC_LAUNCH_CHECK(ctx);
    TC_HIP(ctx, hipMemcpyAsync(chain_path, pathbits, (size_t)chain_words * sizeof(u64), hipMemcpyDeviceToDevice, s));
    TC_HIP(ctx, hipMemcpyAsync(chain_sign, signbits, (size_t)chain_words * sizeof(u64), hipMemcpyDeviceToDevice, s));
    {   // (row blocks that hold a position on path; a block's words are shared by up to 1024 workgroups)
        tc_memset_async(ctx, any, 0, (size_t)cd.nb * sizeof(u32));
        u64 parts = ((u64)cd.bk * cd.h / 64) / 4096 + 1;
        if (parts > 1024) parts = 1024;
        chain_blockany_kernel<<<dim3(cd.nb, (u32)parts), 256, 0, s>>>(chain_path, cd, any);
        TC_LAUNCH_CHECK(ctx);
    }
    const u32 cgrid = (u32)tc_cdiv((u64)cd.nb * cd.h, 256);
    if (cd.nb > 1) {
        chain_scan_a_kernel<<<cgrid, 256, 0, s>>>(chain_path, chain_sign, cd, any, b.chain_summ);
        TC_LAUNCH_CHECK(ctx);
        chain_scan_b_kernel<<<tc_cdiv(cd.h, 256), 256, 0, s>>>(b.chain_summ, cd);
        TC_LAUNCH_CHECK(ctx);
    }
    chain_scan_c_kernel<<<cgrid, 256, 0, s>>>(chain_path, chain_sign, cd, any, b.chain_summ, b.chain_code);
    TC_LAUNCH_CHECK(ctx);
    R.st().chain_rounds++;
    sa_trace_step(R, "chain round: codes", N);
    sa_trace_chain_tables(R, cur, mm, hh, cd, chain_path, chain_sign);
}

// One pass over the R.m members of the active set `cur`, all tied on their first h symbols: a second key per member (its
// rank at + h, or what the chain round at hand calls for), a sort inside the groups, group_kernel.  Leaves the members
// still tied in the other active set, their number in R.m, `cur` flipped, h doubled unless the pass was a chain round's
// first, and the round's statistics.  Host synchronisations: one, plus the segmented sort's.
static void sa_doubling_round(SaRun &R, ChainPolicy &chain, int &cur, u64 &h) {
    tc_ctx *ctx = R.ctx;
    SaBuffers &b = R.b;
    hipStream_t s = R.stream();
    tc_stats &st = R.st();
    const RankLookup &rl = R.rl;
    const bool dense = R.dense;
    const u64 N = R.N, m = R.m;
    const int rbits = R.rbits;
    const u32 mm = (u32)m;
    const u32 hh = h > N ? (u32)N : (u32)h;
    sa_trace_group_sizes(R, cur, mm);
    // dense: the round-0 key buffers are dead; sparse: they hold the sorted keys
    u64 *k2 = dense ? b.k0 : b.sk[0], *k2alt = dense ? b.k1 : b.sk[1];
    u32 *kv = dense ? b.v0 : b.sv[0], *kvalt = dense ? b.v2 : b.sv[1];
    RadixPlan p2;
    p2.add_range(0, rbits);
    p2.add_range(32, 32 + rbits);
    RadixPlanDev pd2;
    pd2.npass = p2.npass;
    for (int p = 0; p < p2.npass; p++) { pd2.shift[p] = p2.shift[p]; pd2.mask[p] = p2.mask[p]; }
    // large rounds: digit histograms on the way; dense: the suffix starts are sorted along
    // (no gather through the active set afterwards)
    const bool seg_round = R.K.seg != 0 && mm >= (u32)R.K.seg_min;
    const bool fuse_hist = mm >= (1u << 20) && !seg_round && chain.keymode == 0;
    const bool vals_idx = dense;
    if (fuse_hist) tc_memset_async(ctx, b.hist, 0, sizeof(u32) * RDX_MAX_PASSES * RDX_BINS);
    const u32 chain_words = (u32)(N / 64 + 1);
    u64 *chain_path = reinterpret_cast<u64 *>(b.chain_ref), *chain_sign = chain_path + chain_words;
    if (chain.start(seg_round, hh, h, N, m)) sa_chain_codes(R, cur, mm, hh, chain_path, chain_sign, chain_words);
    const int keymode = chain.keymode;
    if (keymode == 1) {
        chain_key1_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(b.act[cur][1], b.act[cur][2], chain_path, chain_sign, b.chain_code, mm, k2, vals_idx ? kv : nullptr);
    } else if (keymode == 2) {
        u32 kgrid = tc_cdiv(mm, 256);
        if (kgrid > 65536) kgrid = 65536;
        chain_key2_kernel<<<kgrid, 256, 0, s>>>(b.act[cur][1], b.act[cur][2], chain_path, chain_sign, b.chain_code, rl, mm, hh, k2, vals_idx ? kv : nullptr);
    } else {
        // one lookup per thread for small sets (latency-bound); coarser when histograms are kept
        u32 kgrid = fuse_hist ? tc_cdiv(mm, 256 * 8) : tc_cdiv(mm, 256);
        if (fuse_hist && kgrid > 8192) kgrid = 8192;
        // (a few thousand members looked up by counts inside unsorted buckets: the kernel takes a wave per member)
        if (!fuse_hist && !vals_idx && !rl.isa && !rl.skeys && rl.tkeys && mm <= 65536u) kgrid = tc_cdiv(mm, 4);
        if (fuse_hist) key2_kernel<true><<<kgrid, 256, 0, s>>>(b.act[cur][1], b.act[cur][2], rl, mm, hh, k2, vals_idx ? kv : nullptr, pd2, b.hist);
        else key2_kernel<false><<<kgrid, 256, 0, s>>>(b.act[cur][1], b.act[cur][2], rl, mm, hh, k2, vals_idx ? kv : nullptr, pd2, b.hist);
    }
    TC_LAUNCH_CHECK(ctx);
    sa_trace_step(R, "round: keys (rank lookups)", mm);
    RadixBuffers r2 = sa_radix_buffers(R, k2, k2alt, kv, kvalt);
    if (seg_round) {
        // the members are in SA order, so every group is a run of equal top key halves: a sort inside the runs
        // (tc_seg.hpp) instead of eight stable passes over the whole set
        if (!vals_idx) {
            seg_iota_kernel<<<tc_cdiv(mm, 256), 256, 0, s>>>(kv, mm);
            TC_LAUNCH_CHECK(ctx);
        }
        seg_sort_pairs(ctx, b.seg, k2, kv, k2alt, kvalt, mm, keymode == 1 ? 32 : rbits);
        st.seg_rounds++;
    } else {
        radix_sort_pairs(ctx, r2, mm, p2, /*gen_idx=*/!vals_idx, /*hist_ready=*/fuse_hist);
    }
    sa_trace_step(R, seg_round ? "round: segmented sort" : "round: radix passes", mm);
    GroupArgs gr = {};
    gr.keys = r2.keys; gr.count = mm; gr.vals = r2.vals; gr.vals_are_idx = vals_idx ? 1 : 0;
    gr.in_slot = b.act[cur][0]; gr.in_idx = b.act[cur][1]; gr.in_tpos = b.act[cur][3];
    gr.isa = dense ? b.isa : nullptr; gr.t_rank = dense ? nullptr : b.t_rank;
    gr.out_slot = b.act[cur ^ 1][0]; gr.out_idx = b.act[cur ^ 1][1];
    gr.out_grp = b.act[cur ^ 1][2]; gr.out_tpos = b.act[cur ^ 1][3];
    // dense, large round: ranks by regions (pairs into the scratch key buffer; the sorted keys are dead
    // once the groups are made, so the partitioned pairs go there)
    const bool gr_pairs = dense && mm >= R.bin_min;
    if (gr_pairs) gr.pairs = r2.keys_alt;
    sa_run_group(R, false, gr);
    if (gr_pairs) sa_apply_pairs(R, r2.keys_alt, mm, r2.keys);
    if (keymode != 2) {   // (a chain round is ONE entry -- its first pass's: every entry is a doubling of h, so the rounds stay <= 32)
        st.m[st.rounds] = m; st.key_bytes[st.rounds] = 8; st.passes[st.rounds] = seg_round ? 1u : (u32)p2.npass;
        st.h[st.rounds] = hh;
        st.rounds++;
    } else {
        st.passes[st.rounds - 1]++;
    }
    R.m = sa_fetch_m(R);
    sa_trace_step(R, "round: groups", mm);
    cur ^= 1;
    if (chain.finish(mm, R.m)) h *= 2;
}

static void sa_run(tc_ctx *ctx, SaBuffers &b, const u8 *d_text, u64 n, u32 *d_sa, u8 *d_L,
                   u64 *primary, u32 *counts256_out) {
    const u64 N = n + 1;
    hipStream_t s = ctx->stream;
    tc_stats &st = ctx->stats;
    SaRun R{ctx, b, d_text, n, N, ceil_log2_u64(N), d_sa, d_sa ? d_sa : b.v1, d_L, SaKnobs{}};
    R.rshift = R.rbits > 8 ? R.rbits - 8 : 0;
    R.bin_min = 1ull << R.K.bin_min_log2;   // (below ~2^25 members the direct stores are as fast)
    // (the second active set's slot + idx arrays are adjacent in the arena and together hold N u64)
    R.part_act1 = reinterpret_cast<u64 *>(b.act[1][0]);
    R.part_act1_ok = (size_t)((char *)b.act[1][2] - (char *)b.act[1][0]) >= N * sizeof(u64) &&
                     ((uintptr_t)b.act[1][0] & 7) == 0;
    sa_trace_buffers(R);
    ctx->msd_split_used = 0;
    ctx->msd_dir_used = 0;
    ctx->tied_probe_used = 0;
    ctx->tied_probe_found = 0;
    if (sa_alphabet(R, counts256_out, primary)) return;

    const u32 P_full = R.cfg.P;   // fields chosen for the full path (every field is a pass there)
    R.h_start = R.cfg.h0;
    bool hopeless = false;    // the sample says the tied set would exceed the sparse capacity
    bool many_ties = false;   // the LSD way's finish pass drowned in ties: the full path that follows will want dense ranks
    tc_memset_async(ctx, ctx->d_scalars, 0, 16 * sizeof(u64));
    const bool fast = R.K.finish != 0 && R.K.dense == 0 && sa_round0(R, hopeless, many_ties);
    if (!fast) sa_full_path(R, P_full, hopeless, many_ties);

    R.trace_t0 = std::chrono::steady_clock::now();
    sa_trace_step(R, "(sync before the rank table)", R.m);
    sa_rank_tables(R);
    sa_trace_step(R, R.dense ? "ranks: dense ISA" : "ranks: sparse table", R.m);

    if (R.K.h_start > 0) R.h_start = (u64)R.K.h_start;  // experiments: any h <= sorted depth is valid
    ChainPolicy chain(R.K.chain);
    int cur = 0;
    u64 h = R.h_start;
    while (R.m > 0) {
        if (st.rounds >= TC_MAX_ROUNDS) TC_FAIL(ctx, TC_ERR_INTERNAL, "suffix sort did not converge");
        sa_doubling_round(R, chain, cur, h);
    }
    primary_kernel<<<1, 64, 0, s>>>(R.rl, ctx->d_scalars);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, ctx->h_scalars, ctx->d_scalars, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    *primary = ctx->h_scalars[SA_SLOT_PRIMARY];
    st.sigma = R.cfg.sigma_text + 1;
    st.radix_launches = 0;
    st.ms_radix = 0;
    for (int i = 0; i < ctx->pev_used; i++) {  // stream is idle here (last group sync)
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->pev[2 * i], ctx->pev[2 * i + 1]) == hipSuccess) {
            st.ms_radix += ms;
            st.radix_launches++;
        }
    }
}
