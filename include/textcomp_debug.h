/*
 * textcomp_debug.h -- measurement hooks of libtextcomp.so (not part of the drop-in
 * boundary): calibration micro-kernels used to put the pipeline's kernels next to what
 * the memory system delivers on this device for the same access width.
 */
#ifndef TEXTCOMP_DEBUG_H
#define TEXTCOMP_DEBUG_H
#include "textcomp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* The container's position-dependent 64-bit checksum (checksum64_kernel) of any device range
 * (4-byte aligned, length a multiple of 4): lets a test compare full-size device outputs with
 * a digest computed once by the CPU oracle (tests/golden/c3_digest.json). */
int tc_dbg_checksum64_dev(tc_ctx *ctx, const void *d_p, uint64_t bytes, uint64_t *out);
/* Streams `bytes` from one workspace buffer to another `iters` times and returns the
 * mean copy rate in GB/s (read + write bytes / time).  width: bytes per lane per access
 * (1, 2, 4, 8, 16).  mode 0: copy, 1: read-only (sum), 2: write-only (fill). */
int tc_dbg_stream_bench(tc_ctx *ctx, uint64_t bytes, int width, int mode, int iters, double *gbps);
/* Sorts n random (u64 key, u32 value) pairs by the top `key_bits` key bits with the
 * device radix sort and returns the mean duration of one pass in ms (HIP events).
 * check != 0: verify the result is sorted and stable (returns TC_ERR_INTERNAL if not). */
int tc_dbg_sort_bench(tc_ctx *ctx, uint64_t n, int key_bits, int iters, int check, double *ms_per_pass);
/* The memory pattern of one radix pass alone: 4096-pair tiles read coalesced, written as `bins`
 * segments per tile, each behind the same segment of the previous tile; xrun > 0: blocks on the
 * same XCD take tiles in runs of xrun (the pass's XCD-aware order); mean ms per pass. */
int tc_dbg_scatter_bench(tc_ctx *ctx, uint64_t n, uint32_t bins, uint32_t xrun, int iters, double *ms_per_pass);
/* Where the hardware puts the workgroups of a grid launched on this context's stream: `grid` workgroups of 1024
 * threads with `lds_bytes` of LDS each (147456: one per CU) spin for `spin_cycles`; out6[6 * grid] (host)
 * receives per workgroup: XCC id, HW_ID register, start (2 words, 100 MHz wall clock), duration, scratch. */
int tc_dbg_dispatch_probe(tc_ctx *ctx, uint32_t grid, uint32_t lds_bytes, uint32_t spin_cycles, uint32_t *out6);
/* The short cap of the LCP array's one-lane compare kernel (csrc/tc_lcp.hpp: comparisons that reach it go on, one
 * workgroup each) for the later tc_lcp_array / tc_lcp_array_dev calls of this context: a multiple of 16 in 16 .. 65536,
 * or 0 for the library's TC_LCP_SHORT_CAP.  The results do not depend on it; scripts/lcp_bench.py sweeps it. */
int tc_dbg_lcp_set_short_cap(tc_ctx *ctx, uint32_t cap);
/* The fan-out of the min tree over the LCP array (csrc/tc_fm_ms.hpp) of the indexes the later tc_fm_build_lcp /
 * tc_fm_build_lcp_dev calls of this context make: 4, 8, 16 or 64 (the library's FM_LCP_FANOUT); anything else is
 * TC_ERR_ARG.  The fan-out is stored in the index; the results do not depend on it.  It exists so that tests reach every
 * level of the tree at a thousand rows. */
int tc_dbg_fm_set_lcp_fanout(tc_ctx *ctx, uint32_t fanout);
/* The positions per tile of the phrase-start steps of the later tc_lz_parse / tc_lz_parse_dev calls of this context
 * (csrc/tc_lz.hpp): a power of two in 64 .. 16384, or 0 for the library's LZ_TILE; anything else is TC_ERR_ARG.  The
 * results do not depend on it.  It exists so that tests reach tile boundaries at a few thousand bytes.  (The two min
 * trees of those calls have the fan-out tc_dbg_fm_set_lcp_fanout set.) */
int tc_dbg_lz_set_tile(tc_ctx *ctx, uint32_t tile);
/* *used = 1 if round 0 of this context's last suffix sort (an encode runs one) went the MSD way with levels 1 and 2 in
 * the split key layout (csrc/tc_msd.hpp: two arrays of 32-bit key halves; TC_MSD_SPLIT), 0 if not -- the LSD way, levels
 * that move suffix starts, TC_SA_MSD_JOINT=0, or a second run of the levels with suffix starts. */
int tc_dbg_msd_split_used(tc_ctx *ctx, uint32_t *used);
/* out[0] = 1 if round 0 of this context's last suffix sort went the MSD way and its aligned level (level 3 with the joint
 * table) kept the directory of its live parents in LDS (csrc/tc_msd.hpp, csrc/tc_msd_dir.hpp; TC_MSD_DIR), 0 if not -- the
 * LSD way, TC_SA_MSD_JOINT=0, TC_MSD_DIR=0.  out[1] = the fills of that directory, summed over the workgroups (one per
 * round of slots a workgroup looked at; 0 where out[0] is 0). */
int tc_dbg_msd_dir(tc_ctx *ctx, uint32_t out[2]);
/* The pass over the text that finds the tied suffixes of key-only MSD levels again (csrc/tc_sa.hpp; TC_TIED_PROBE), of this
 * context's last suffix sort.  out[0] = 0 if none ran (the LSD way, levels that move suffix starts, no tied suffix, more
 * than the table is made for), 1 = tied_probe_kernel (codes through a byte image in LDS), 2 = tied_probe_w_kernel (raw text
 * in LDS, codes from the key generator's register table).  out[1] = the entries it found (0 where out[0] is 0).  When the
 * levels ran a second time with suffix starts, the figures are those of the key-only attempt before it. */
int tc_dbg_tied_probe(tc_ctx *ctx, uint32_t out[2]);
/* What the splitter walks of this context's last inverse BWT (a decode runs one; csrc/tc_ibwt.hpp, ibwt_walk_rank_copy in
 * csrc/tc_decode_host.hpp) did.  out[0] = the attempts run: 1, or 2 when the walks of the first wanted more extra splitter
 * slots than there are and were repeated the old way; 0 if no walk ran (a column without a Nothing).  Of the last attempt:
 * out[1] = the records that overflowed (their segments are walked a second time; TC_IBWT_REWALK=1 marks every record so),
 * out[2] = the extra slots asked for by walks whose record filled up (TC_IBWT_SEGCAP lowers that fill; more than the
 * K / 32 + 256 slots of K splitters only in a first attempt that was then repeated). */
int tc_dbg_ibwt_walk(tc_ctx *ctx, uint32_t out[3]);
/* The sort of one doubling round (seg_sort_pairs, csrc/tc_sa_host.hpp; kernels in csrc/tc_seg.hpp) on the caller's pairs,
 * staged through the context's workspace with the run and tile tables a text of m suffixes gets.  keys[i] = grp << 32 | rank,
 * grp non-decreasing, rank < 2^rbits (rbits 1 .. 32); 1 <= m <= 2^24; all host arrays.  On return keys / vals hold the
 * result: inside every run of equal grp the members ordered by rank.  Members with equal keys come in no defined order.
 * levels[2L], levels[2L + 1] = the long runs (above 1024 members) and the 4096-member tiles the host read back before
 * partition level L (L < 8); zeros after the last.  TC_ERR_ARG: a null pointer, m or rbits out of range, a grp that
 * decreases, a rank of more than rbits bits -- nothing ran.  TC_ERR_INTERNAL: runs left after 8 levels. */
int tc_dbg_seg_sort(tc_ctx *ctx, uint64_t *keys, uint32_t *vals, uint32_t m, int rbits, uint32_t levels[16]);
/* tied_small_kernel<mode> (csrc/tc_seg.hpp: one workgroup, the same network) on 1 <= m <= 4096 members; all host arrays.
 * mode 0: (slot, idx, grp) sorted by slot in place, entries with slot = 0xffffffff last; t_idx / t_rank / tpos ignored.
 * mode 1: slot is not looked at; idx distinct; t_idx = idx sorted, t_rank[c] = grp of the member at row c, tpos[k] = the row
 * of member k -- as table_build_kernel (csrc/tc_sa.hpp) defines them; slot / idx / grp unchanged.
 * TC_ERR_ARG: another mode, m out of range, a null pointer among those the mode uses. */
int tc_dbg_tied_small(tc_ctx *ctx, int mode, uint32_t *slot, uint32_t *idx, uint32_t *grp, uint32_t m,
                      uint32_t *t_idx, uint32_t *t_rank, uint32_t *tpos);
#ifdef __cplusplus
}
#endif
#endif
