// tc_msd_dir.hpp -- the tile cursor of an aligned MSD level (tc_msd.hpp: level 3 with the joint table) over a DIRECTORY of
// the workgroup's live parents.  Plain C++ without a HIP header: the partition kernel uses msd_dir_next as it stands, and
// host/check/msd_dir_walk.cpp drives all of it under a host sanitizer against a transcription of the old walk.
//
// A workgroup of an aligned level owns the parent slots [q0, q1); most are empty (1 GiB ACGTN: 61 live of 256).  The
// directory holds (parent, pstart, pcnt) of the live ones, in slot order, as many as fit; a fill looks at the next
// MSD_DIR_BATCH slots per round and goes on until it has found a live one or the slots are used up.  The cursor hands out
// the tiles of the entries one after the other -- ceil(pcnt / tile) each, so no table of tile numbers is read -- and says
// "pending" when it runs past the filled entries while slots remain: the kernel then refills at the next end of a
// segment, where all its threads meet anyway, and asks again for the tiles that were pending.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MSD_DIR_FN __host__ __device__ __forceinline__
#else
#define MSD_DIR_FN static inline
#endif

#define MSD_DIR_NONE 0xffffffffu
#define MSD_DIR_PENDING 2u   // `last` of a tile description that is not known yet (valid = 0)
#define MSD_DIR_BATCH 1024u  // slots a fill looks at per round in the default build (the partition kernel: one per thread, MSD_NT)

struct MsdDirEnt {
    uint32_t q, ps, pc;   // parent, its first position, its count (> 0)
};
struct MsdDirTile {       // the fields of MsdTileInfo (tc_msd.hpp)
    uint32_t base, valid, q, last;
};
struct MsdDirCur {
    uint32_t e, k;          // the next tile: tile k of entry e
    uint32_t n;             // filled entries
    uint32_t qnext, qend;   // slots not looked at yet: [qnext, qend)
    uint32_t pend;          // tiles asked for since the walk ran past the filled entries with slots remaining
};

// The next tile.  *nq: the parent of the entry behind the tile's own (MSD_DIR_NONE: none, or not filled yet).
// Past the last entry: valid = 0, and last = MSD_DIR_PENDING if slots remain (the tile may exist), 0 if not.
MSD_DIR_FN void msd_dir_next(const MsdDirEnt *dir, MsdDirCur &c, const uint32_t tile, MsdDirTile *out, uint32_t *nq) {
    *nq = MSD_DIR_NONE;
    if (c.e >= c.n) {
        out->base = 0; out->valid = 0; out->q = 0; out->last = 0;
        if (c.qnext < c.qend) { out->last = MSD_DIR_PENDING; c.pend++; }
        return;
    }
    const MsdDirEnt d = dir[c.e];
    const uint32_t off = c.k * tile, left = d.pc - off;
    out->base = d.ps + off;
    out->valid = left < tile ? left : tile;
    out->q = d.q;
    out->last = left <= tile ? 1u : 0u;
    if (c.e + 1 < c.n) *nq = dir[c.e + 1].q;
    if (left <= tile) { c.e++; c.k = 0; } else c.k++;
}

// ---- the rest is the host's model of what the kernel does around the cursor (msd_partition_body, DIR) -------------
// One round of a fill: the live slots among the next `batch`, as many as fit.
static inline void msd_dir_fill_round(MsdDirEnt *dir, MsdDirCur &c, uint32_t cap, uint32_t batch, const uint32_t *pcnt,
                                      const uint32_t *pstart) {
    uint32_t q = c.qnext;
    const uint32_t hi = c.qend - q < batch ? c.qend : q + batch;
    for (; q < hi; q++) {
        if (pcnt[q] == 0) continue;
        if (c.n == cap) break;   // the first live slot that does not fit: the next fill starts here
        dir[c.n].q = q; dir[c.n].ps = pstart[q]; dir[c.n].pc = pcnt[q];
        c.n++;
    }
    c.qnext = q;
}
// A fill (only ever when nothing filled lies ahead of the cursor); returns the rounds it took.
static inline uint32_t msd_dir_refill(MsdDirEnt *dir, MsdDirCur &c, uint32_t cap, uint32_t batch, const uint32_t *pcnt,
                                      const uint32_t *pstart) {
    uint32_t rounds = 0;
    c.e = 0; c.k = 0; c.n = 0; c.pend = 0;
    while (c.n == 0 && c.qnext < c.qend) {
        msd_dir_fill_round(dir, c, cap, batch, pcnt, pstart);
        rounds++;
    }
    return rounds;
}
// The tiles of the slots [q0, q1) in the order the kernel works on them, with its look-ahead of three tiles through a
// ring of four descriptions, refills at ends of segments only.  out[max_out]; returns the number of tiles (which may
// exceed max_out: the rest is not stored), *fills = rounds of all fills.  *bad is raised if the protocol breaks: a
// pending description reaches the head of the ring, or a description is pending behind a tile that is not a last one.
static inline uint64_t msd_dir_walk(const uint32_t *pcnt, const uint32_t *pstart, uint32_t q0, uint32_t q1, MsdDirEnt *dir,
                                    uint32_t cap, uint32_t batch, uint32_t tile, MsdDirTile *out, uint64_t max_out,
                                    uint32_t *fills, int *bad) {
    MsdDirCur c = {0, 0, 0, q0, q1, 0};
    MsdDirTile ring[4];
    uint32_t nq;
    uint64_t t = 0;
    *bad = 0;
    *fills = msd_dir_refill(dir, c, cap, batch, pcnt, pstart);
    for (int i = 0; i < 3; i++) msd_dir_next(dir, c, tile, &ring[i], &nq);
    for (;; t++) {
        const MsdDirTile ti = ring[t & 3];
        if (ti.valid == 0) {
            if (ti.last == MSD_DIR_PENDING) *bad = 1;
            break;
        }
        msd_dir_next(dir, c, tile, &ring[(t + 3) & 3], &nq);
        const uint32_t dpend = c.pend;
        if (t < max_out) out[t] = ti;
        if (dpend == 3 && !ti.last) *bad = 1;
        if (ti.last && dpend) {
            *fills += msd_dir_refill(dir, c, cap, batch, pcnt, pstart);
            for (uint64_t x = t + 4 - dpend; x <= t + 3; x++) msd_dir_next(dir, c, tile, &ring[x & 3], &nq);
        }
    }
    return t;
}
