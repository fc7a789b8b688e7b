/*
 * textcomp.h -- C ABI of libtextcomp.so: the MI355X (gfx950) BWT -> MTF -> RLE /
 * FM-index hot path behind the Data.BWT / Data.MTF / Data.RLE / Data.FMIndex
 * module surface of Matthew-Mosior/text-compression (v0.1.0.25).
 *
 * The reference has no FFI of its own (not one `foreign import`); these entry
 * points are what a Haskell shim's `foreign import ccall safe` would bind in
 * place of the L2 `Seq (Maybe a)` kernels (INTEGRATION.md shows the stubs).
 * Each function cites the reference function(s) it replaces, paths relative to
 * the reference's src/Data/.
 *
 * Conventions
 *   - plain C: pointers and sizes only; no C++/torch types; no exceptions.
 *   - `Maybe Word8` <-> int16_t, -1 = Nothing (order -1 < 0 < .. < 255 equals
 *     `Ord (Maybe Word8)`).  A BWT is `uint8_t L[N]` + `primary` = the slot that
 *     holds Nothing (its byte in L is 0).  N = n + 1; n == 0 <=> N == 0
 *     (BWT.hs:58: empty input gives an empty BWT, no lone sentinel).
 *   - caller allocates and frees every input/output buffer; the library owns only
 *     tc_ctx / tc_fm handles.  Variable-size outputs use in/out capacity words.
 *   - return 0 = TC_OK, negative = error; tc_last_error(ctx) has the text.
 *     TC_ERR_MALFORMED marks inputs on which the reference itself throws
 *     (fromJust / DS.index / read).
 *   - one tc_ctx = one device + one HIP stream + one workspace; calls on one ctx
 *     are serialised by the caller, distinct ctxs are independent: calls on
 *     distinct ctxs may run at the same time from different threads, on one
 *     device, and ctxs may be created and destroyed meanwhile
 *     (tests/test_gpu_concurrency.py).  A tc_fm is read-only once built: count
 *     and locate carve their scratch from the CALLING ctx's workspace, so any
 *     number of ctxs on the index's device may query one tc_fm at the same
 *     time; tc_fm_free must not overlap a query of that index.  The same holds
 *     for tc_fm_locate_dev and for a sampled index (tc_fm_build_sampled): the
 *     walk's scratch and its error flag belong to the calling ctx; and for
 *     tc_fm_extract / tc_fm_extract_dev on an index with text samples.
 *   - `*_dev` entry points take DEVICE pointers for the bulk arrays (the
 *     benchmark path: inputs and outputs resident in HBM); scalar outputs are
 *     host words.  All calls return after the ctx stream has drained.
 *   - limits: n <= TC_MAX_N.  There is NO CPU fallback: without a usable HIP
 *     device every compute call fails with TC_ERR_HIP.
 */
#ifndef TEXTCOMP_H
#define TEXTCOMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TC_OK 0
#define TC_ERR_ARG (-1)
#define TC_ERR_CAPACITY (-2)
#define TC_ERR_MALFORMED (-3)
#define TC_ERR_HIP (-4)
#define TC_ERR_OOM (-5)
#define TC_ERR_INTERNAL (-6)
#define TC_ERR_NCCL (-7)     /* RCCL missing or failing (tc_comm_* only) */

#define TC_MAX_N ((uint64_t)0x7ffffff0u) /* indices are 31-bit on the device */
#define TC_MAX_SIGMA 257                 /* 256 byte values + Nothing */
#define TC_MAX_ROUNDS 40

typedef struct tc_ctx tc_ctx;
typedef struct tc_fm tc_fm;

/* Work counters of the last encode on this ctx: the inputs of the algorithmic-
 * byte formula of SURVEY.md 8(d) / DESIGN.md, plus per-stage device time. */
typedef struct tc_stats {
    uint64_t n;                      /* input bytes */
    uint64_t N;                      /* n + 1 */
    uint32_t sigma;                  /* present symbols incl. Nothing */
    uint32_t rounds;                 /* suffix-sort rounds executed (round 0 = k-mer sort) */
    uint64_t m[TC_MAX_ROUNDS];       /* suffixes sorted in round r (m[0] = N) */
    uint32_t key_bytes[TC_MAX_ROUNDS];   /* k_r: key bytes moved per element */
    uint32_t passes[TC_MAX_ROUNDS];      /* P_r: radix passes */
    uint32_t h[TC_MAX_ROUNDS];           /* symbols resolved entering round r */
    uint64_t runs;                   /* RLE runs produced */
    float ms_sa, ms_bwt, ms_mtf, ms_rle, ms_total; /* device time, HIP events */
    /* dominant kernel (one radix-sort pass over all N suffixes), timed with HIP
     * events on the ctx stream when tc_ctx_set_profile(ctx, 1) is on */
    uint32_t radix_launches;         /* round-0 pass launches timed */
    float ms_radix;                  /* their summed duration */
    uint32_t keygen_fused;           /* 1: the first pass builds its keys from the text (reads 1 B,
                                        writes 12 B per suffix instead of 12 + 12) */
    uint32_t finish_pass;            /* 1: round 0 = partial sort + finish kernel (12 B read, 5 B written) */
    uint32_t sample_dups;            /* of 8192 sampled suffixes, how many repeated another sample's
                                        globally sorted prefix (> 10 %: full path without trying the
                                        finish pass) */
    uint32_t msd_path;               /* 1: round 0 ran as the MSD partition levels + bucket finish (tc_msd.hpp:
                                        long texts over a small alphabet); radix_launches / ms_radix then time
                                        msd_partition_kernel (first launch reads the text: 1 + 12 B per suffix,
                                        the others 12 + 12 B) */
    uint32_t msd_keyonly;            /* 1: the MSD levels moved keys only (no suffix array was asked for: encode, BWT):
                                        8 + 8 B per suffix per level (the first: 1 + 8) instead of 12 + 12; the suffix starts
                                        of the tied set were found again by one pass over the text */
    uint32_t ticket_fallbacks;       /* suffix sorts of this ctx that had to be redone with the single tile-ticket
                                        counter because a look-back of the XCD-grouped ticket order ran into its
                                        spin limit (LSD passes only; 0 in a healthy run, cumulative per ctx) */
    /* Layout note: fields are only ever APPENDED from round 4 on (round 3 put msd_keyonly in front of
     * ticket_fallbacks: callers built against the round-2 header must be rebuilt). */
    uint32_t ws_chunks;              /* physical chunks the context's workspace is mapped from (0: one hipMalloc block) */
    uint32_t ws_grown;               /* how often that workspace grew in place (more chunks mapped; cumulative per ctx) */
    uint32_t seg_rounds;             /* doubling rounds whose sort was the segmented one (tc_seg.hpp), last suffix sort */
    uint32_t chain_rounds;           /* doubling rounds run as chain rounds (tc_chain.hpp: periodic text), last suffix sort; each is ONE
                                        entry of m[] / h[] with passes[] = 2 (was reserved0: same layout) */
} tc_stats;

/* The encoded block of the fused BWT -> MTF -> RLE pipeline.  The reference has
 * no such container (it never feeds MTF output into RLE); this is
 * the documented glue: RLE runs over the MTF index stream as plain integers, with
 * the BWT primary index and the MTF final list (MTF/Internal.hs:125,140-141)
 * carried in the header.
 * Decode treats `primary` as a hint: the Nothing in the index stream decides (the
 * reference's decode takes no primary).  A wrong one costs time, not correctness. */
typedef struct tc_block {
    uint64_t n;                          /* out: input length */
    uint64_t primary;                    /* out: BWT slot of Nothing (decode: a hint) */
    uint32_t sigma;                      /* out: MTF alphabet size */
    int16_t final_list[TC_MAX_SIGMA];    /* out: MTF list after the last move */
    uint64_t nruns;                      /* in: capacity of the run arrays; out: runs */
    uint32_t *run_count;                 /* [capacity] run lengths */
    uint16_t *run_value;                 /* [capacity] MTF index of each run */
} tc_block;

/* ---- context ------------------------------------------------------------ */
int tc_ctx_create(int device, tc_ctx **out);
void tc_ctx_destroy(tc_ctx *ctx);
const char *tc_last_error(const tc_ctx *ctx);
const char *tc_version(void);
int tc_get_stats(const tc_ctx *ctx, tc_stats *out);
/* Stream the ctx launches on (a hipStream_t), for callers that time or order
 * work against it. */
void *tc_ctx_stream(const tc_ctx *ctx);
/* on != 0: bracket every round-0 radix pass with HIP events (tc_stats.ms_radix). */
int tc_ctx_set_profile(tc_ctx *ctx, int on);
/* Workspace placement.  Where the context's workspace lands in device memory decides which of two speeds the
 * partition levels of a long record run at (1 GiB ACGTN on MI355X: 28.9 or 31.0 ms per encode, fixed for the
 * life of the workspace).  This call encodes the caller's representative record
 * (arguments as tc_encode_dev; `out` is overwritten) on up to `tries` differently placed workspaces -- a
 * rejected block stays allocated until the call ends, so that the next one lands elsewhere; blocks are only
 * added while device memory has room for them -- and keeps the fastest.  ms (host, [tries], optional)
 * receives the encode time per placement (0 = not tried), *chosen its index.  Not part of the reference's
 * surface: a set-up step for long-lived contexts, before any timed work. */
int tc_ctx_place_workspace(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_block *out, int tries, double *ms,
                           int *chosen);

/* ---- Data.BWT ------------------------------------------------------------ */
/* bytestringToBWT (BWT.hs:68-70) = toBWT (:55-64) = createSuffixArray
 * (BWT/Internal.hs:110-134) + saToBWT (:98-106).  L has n+1 bytes. */
int tc_bwt_encode(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *L, uint64_t *primary);
int tc_bwt_encode_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint8_t *d_L,
                      uint64_t *primary);
/* createSuffixArray alone: sa[j] = 0-based start of the j-th smallest suffix of
 * text.'$' (reference: 1-based suffixstartpos), n+1 entries. */
int tc_suffix_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sa);
/* The same with text and array resident in HBM: d_sa receives n+1 entries (n == 0: the one entry 0, as above).
 * Not part of the reference's surface, like the three calls below. */
int tc_suffix_array_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_sa);
/* The LCP array that goes with that suffix array (together: the enhanced suffix array).  lcp has n+1 entries:
 * lcp[0] = 0, and for j >= 1 lcp[j] = length of the longest common prefix of the suffixes starting at sa[j-1] and
 * sa[j].  The end of the text matches nothing, so lcp[j] <= n - max(sa[j-1], sa[j]) and lcp[1] = 0.  n == 0 writes
 * lcp[0] = 0 (and sa[0] = 0).
 *   tc_lcp_array      sorts and computes in one call; sa (host, n+1 entries) may be NULL.
 *   tc_lcp_array_dev  takes a suffix array that already lies in HBM (tc_suffix_array_dev's, or one the caller kept).
 *                     d_text holds exactly n bytes: nothing before or behind them is read.  A d_sa that is not a
 *                     permutation of 0..n (an entry above n, a value twice, a value missing): TC_ERR_MALFORMED, every
 *                     read and write in bounds; a permutation that is not the suffix array of d_text: values without
 *                     meaning, each still <= n - max(sa[j-1], sa[j]), no error.  n == 0: d_sa is not read.
 * Null buffers or n > TC_MAX_N: TC_ERR_ARG.  Scratch (4 bytes per entry, plus at most another 4 n for comparisons
 * longer than a few hundred bytes) comes from the calling ctx's workspace. */
int tc_lcp_array_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint32_t *d_sa, uint32_t *d_lcp);
int tc_lcp_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sa, uint32_t *lcp);
/* One reduction over N entries of an LCP array in HBM: *max_lcp = the largest entry, *row = the smallest row that
 * holds it (rows row-1 and row of the suffix array are the longest repeat), *sum = the sum of all entries (the text
 * has n(n+1)/2 - sum distinct substrings).  N == 0: TC_ERR_ARG. */
int tc_lcp_summary_dev(tc_ctx *ctx, const uint32_t *d_lcp, uint64_t N, uint32_t *max_lcp, uint64_t *row, uint64_t *sum);
/* ---- the LZ77 parse of a text against itself (not part of the reference's surface) ----
 * lcp(i, j) = the length of the longest common prefix of text[i..n) and text[j..n); the end of the text matches nothing.
 * THE LPF ARRAY, n entries, all positions 0-based: lpf[i] = the maximum of lcp(i, j) over j < i (0 for i = 0); the source
 * may overlap the phrase (j + lpf[i] > i is allowed).  src[i]: among the suffixes that start before i, suffix i has two
 * lexicographic neighbours -- the largest that is smaller and the smallest that is larger (in suffix-array order the end
 * of the text sorts first); src[i] is the start of the one that shares the longer prefix with suffix i, on a tie of the
 * smaller one, and 0 where lpf[i] = 0.  src (d_src) may be NULL.
 * THE PARSE is greedy, left to right: at position i, lpf[i] = 0 gives the literal phrase (ph_src = text[i], ph_len = 0)
 * and i += 1; otherwise the copy phrase (ph_src = src[i], ph_len = lpf[i]) and i += lpf[i].  ph_len = 0 marks literals, as
 * in tc_fm_factorize.  The empty text has 0 phrases; 64 times "a" parses to (97, 0), (0, 63).  *nph: in = capacity of
 * the two arrays, out = the phrase count.  A capacity that is too small: TC_ERR_CAPACITY, *nph = the needed count, nothing
 * written to the arrays.  ph_src = ph_len = NULL with capacity 0 is the sizes-only form: TC_OK, the count written.
 * THE INVERSE: a copy phrase that starts at output position s copies text[ph_src + k] to text[s + k] for k = 0 .. len - 1
 * in increasing order, so an overlapping source is well defined; tc_lz_unparse(tc_lz_parse(text)) = text for every byte
 * string.  *nbytes: in = capacity of text, out = the bytes; too small: TC_ERR_CAPACITY, *nbytes = the needed count, nothing
 * written; text = NULL with capacity 0 is the sizes-only form.  A bad phrase list -- a copy with ph_src >= its own start
 * position, a literal with ph_src > 255, a total above TC_MAX_N -- is TC_ERR_ARG with nothing written to text.
 * ERRORS AND EDGES.  Null buffers or n > TC_MAX_N: TC_ERR_ARG.  n = 0: TC_OK, 0 phrases, nothing read or written.
 * nph = 0: 0 bytes.  The parse and LPF calls take the text only: the suffix array, the LCP array and all scratch (20 bytes
 * per text byte behind the sort: sa 4, lcp 4, (lpf, src) 8, the tiles' exits 4; the sort's own need where that is larger)
 * live in the calling ctx's workspace.
 * The _dev forms take every array in HBM; nph and nbytes stay host words.  The unparse scratch is at most 24 bytes per phrase
 * and 8 bytes per byte of the text (not of the capacity). */
int tc_lpf_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *lpf, uint32_t *src);
int tc_lpf_array_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_lpf, uint32_t *d_src);
int tc_lz_parse(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *ph_src, uint32_t *ph_len, uint64_t *nph);
int tc_lz_parse_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_ph_src, uint32_t *d_ph_len, uint64_t *nph);
int tc_lz_unparse(tc_ctx *ctx, const uint32_t *ph_src, const uint32_t *ph_len, uint64_t nph, uint8_t *text, uint64_t *nbytes);
int tc_lz_unparse_dev(tc_ctx *ctx, const uint32_t *d_ph_src, const uint32_t *d_ph_len, uint64_t nph, uint8_t *d_text,
                      uint64_t *nbytes);
/* ---- the maximal and supermaximal repeats of a text (not part of the reference's surface) ----
 * N = n + 1 rows; sa and lcp as tc_lcp_array defines them (row 0 is the empty suffix, the end of the text matches
 * nothing).  left(r) = text[sa[r] - 1], and Nothing -- which differs from every byte -- for the one row with sa[r] = 0.
 * A REPEAT is a string of length l >= 1 that occurs at least twice; occurrences may overlap.  It is MAXIMAL if extending
 * all its occurrences by one byte to the right does not keep them all equal (the end of the text counts as a byte that
 * differs from everything), and the same to the left (the start of the text).  In rows: an LCP interval [lb, rb], lb < rb,
 * l = min lcp[lb+1 .. rb] >= 1, lcp[lb] < l, rb = N - 1 or lcp[rb+1] < l, whose left(lb .. rb) are not all equal.  It is
 * SUPERMAXIMAL if it is a substring of no other maximal repeat: lcp[k] = l for every k in lb+1 .. rb and left(lb .. rb)
 * pairwise distinct, so it occurs at most 257 times.  "mississippi": maximal i x4, issi x2, p x2, s x4; supermaximal issi, p.
 * OUTPUT, per repeat: rep_row = lb, rep_pos = sa[lb] (0-based: the occurrence whose suffix sorts first), rep_len = l,
 * rep_occ = rb - lb + 1; all occurrences of repeat k are sa[rep_row[k] .. rep_row[k] + rep_occ[k]).  sa (n + 1 entries)
 * and rep_row may each be NULL.  ORDER: every interval is reported once, from its representative row j = the smallest
 * row in (lb, rb] with lcp[j] = l, in increasing j.  That is deterministic and, for equal lb, decreasing len; it is NOT
 * sorted by lb.  "aaabaab" has sa = 7 0 4 1 5 2 6 3 and lcp = 0 0 2 3 1 2 0 1; its maximal repeats are the three
 * intervals [1, 3] of "aa" (j = 2), [2, 3] of "aab" (j = 3) and [1, 5] of "a" (j = 4), so rep_row = 1, 2, 1,
 * rep_len = 2, 3, 1, rep_occ = 3, 2, 5 and rep_pos = 0, 4, 0.
 * FILTERS: only repeats with len >= min_len and occ >= min_occ are reported.  min_len = 0, min_occ < 2 or a kind other
 * than the two: TC_ERR_ARG.
 * *nrep: in = capacity of the four arrays, out = the count.  Too small: TC_ERR_CAPACITY, *nrep = the needed count, nothing
 * written to the four arrays (sa, when given, may already be written).  rep_pos = rep_len = rep_occ = NULL with
 * capacity 0 is the sizes-only form: TC_OK, the count written.  A text of n bytes has fewer than n maximal repeats, so
 * capacity n is always enough.
 * ERRORS AND EDGES.  Null buffers or n > TC_MAX_N: TC_ERR_ARG.  n = 0: TC_OK, 0 repeats, nothing read; sa, when given,
 * receives its one entry 0.  The calls take the text only: the suffix array, the LCP array, the last column and all
 * scratch (25 bytes per text byte behind the sort: sa 4, lcp 4, last column 1, the packed rows 8, the left-context change
 * counts 8; the sort's own need where that is larger) live in the calling ctx's workspace.  The _dev form takes every
 * array in HBM; nrep stays a host word. */
#define TC_REPEAT_MAXIMAL 0
#define TC_REPEAT_SUPERMAXIMAL 1
int tc_repeats(tc_ctx *ctx, const uint8_t *text, uint64_t n, int kind, uint32_t min_len, uint32_t min_occ,
               uint32_t *sa, uint32_t *rep_pos, uint32_t *rep_len, uint32_t *rep_occ, uint32_t *rep_row, uint64_t *nrep);
int tc_repeats_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, int kind, uint32_t min_len, uint32_t min_occ,
                   uint32_t *d_sa, uint32_t *d_rep_pos, uint32_t *d_rep_len, uint32_t *d_rep_occ, uint32_t *d_rep_row, uint64_t *nrep);
/* ---- tandem repeats: the runs (maximal repetitions) of a text (not part of the reference's surface) ----
 * A RUN of text[0..n) is a triple (start s, end e, period p), with p >= 1 and 0 <= s <= e < n, such that all of these hold:
 *   - text[k] = text[k+p] for every s <= k <= e - p;
 *   - e - s + 1 >= 2p;
 *   - p is the smallest period of text[s..e];
 *   - the run extends neither way: s = 0 or text[s-1] != text[s+p-1], and e = n - 1 or text[e+1] != text[e+1-p].
 * The ends of the text match nothing.  "mississippi" has the runs (1,7,3), (2,3,1), (5,6,1), (8,9,1); "aabaabaab" has
 * (0,1,1), (0,8,3), (3,4,1), (6,7,1); a unary text of n >= 2 bytes has the single run (0, n-1, 1).  A text of n bytes has
 * fewer than n runs (the runs theorem), so capacity n is always enough.
 * OUTPUT: three arrays run_start = s, run_len = e - s + 1 and run_period = p, in increasing start and, for equal starts,
 * increasing period.  The order depends on the text only, not on the method, and is the same on every call.
 * FILTERS: a run is reported if it passes all four: run_period >= min_period (>= 1); run_period <= max_period, where 0
 * means no limit and any other value must be >= min_period; run_len / run_period, rounded down, >= min_copies (>= 2);
 * run_len >= min_len (>= 1).  Anything else: TC_ERR_ARG.
 * *nrun: in = capacity of the three arrays, out = the count.  Too small: TC_ERR_CAPACITY, *nrun = the needed count, nothing
 * written to the three arrays.  run_start = run_len = run_period = NULL with capacity 0 is the sizes-only form: TC_OK, the
 * count written.
 * ERRORS AND EDGES.  Null buffers or n > TC_MAX_N: TC_ERR_ARG.  n = 0: TC_OK, 0 runs, nothing read.  The calls take the
 * text only: the enhanced suffix arrays of the text and of its reverse and all scratch (66 bytes per text byte behind the
 * two sorts: the two texts 2, one suffix array 4, two inverse suffix arrays, one complement and two LCP arrays 20, the
 * candidate words 24, the per-start counts and segment starts 16; the sort's own need behind the first 26 where that is
 * larger) live in the calling ctx's workspace.  The _dev form takes every array in HBM; nrun stays a host word. */
int tc_tandem_repeats(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_period, uint32_t max_period,
                      uint32_t min_copies, uint32_t min_len, uint32_t *run_start, uint32_t *run_len, uint32_t *run_period,
                      uint64_t *nrun);
int tc_tandem_repeats_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_period, uint32_t max_period,
                          uint32_t min_copies, uint32_t min_len, uint32_t *d_run_start, uint32_t *d_run_len,
                          uint32_t *d_run_period, uint64_t *nrun);
/* ---- palindromes and inverted repeats of a text, with mismatches (not part of the reference's surface) ----
 * sigma is a byte map that is an involution: sigma(sigma(x)) = x for all 256 bytes.  comp is a HOST pointer to its 256
 * bytes, or NULL for the identity; it is a host pointer in the _dev forms too, like the scalar filters.  Under the identity
 * the calls find the palindromes of the text, under the DNA complement (A<->T, C<->G) its inverted repeats: the stretches
 * that equal their own reverse complement.
 * text[s .. s+len) is a SIGMA-PALINDROME with mm mismatches when mm = |{k : 0 <= k < ceil(len/2), text[s+k] !=
 * sigma(text[s+len-1-k])}|.  The middle byte of an odd length counts as a pair with itself: under the DNA complement it
 * is always a mismatch, under the identity it never is.  Its CENTRE is c = 2s + len - 1, which lies in 0 .. 2n-2.
 * For a budget max_mismatch = m the calls report, for every centre, the LONGEST palindrome there that meets all three:
 * mm <= m; its outermost pair matches (a palindrome never ends on a mismatch); len >= min_len.  That is at most one
 * palindrome per centre, so fewer than 2n in all: capacity 2n - 1 is always enough.
 * "mississippi" under the identity with m = 0 and min_len = 3: (1,4,0) issi, (1,7,0) ississi, (4,4,0) issi, (7,4,0) ippi
 * -- sis and ssiss share the centre of ississi and are not reported; with min_len = 1 the ten single bytes that are no
 * longer palindrome's centre join them.  "ACGT" under the DNA complement: (0,4,0) alone -- CG shares its centre.  "ACAGT"
 * under the DNA complement: nothing at m = 0; (0,5,1) and (2,3,1) at m = 1 -- AGT, like every odd length, spends one
 * mismatch on its middle byte.
 * OUTPUT: three arrays pal_start = s, pal_len = len and pal_mm = mm, in increasing centre.  pal_mm alone may be NULL in any
 * call; it is then not written.
 * *npal: in = capacity of the arrays, out = the count.  Too small: TC_ERR_CAPACITY, *npal = the needed count, nothing
 * written to the arrays.  pal_start = pal_len = pal_mm = NULL with capacity 0 is the sizes-only form: TC_OK, the count
 * written.
 * tc_longest_palindrome: the longest palindrome under the same rule (min_len = 1), of equal lengths the one with the
 * smallest centre, into three host words in both forms.  len = 0 when there is none: n = 0, or a sigma without a fixed
 * point and a text without a matching pair.
 * ERRORS AND EDGES.  TC_ERR_ARG, before a buffer is touched, for: a null npal; a null required buffer; min_len = 0;
 * max_mismatch > TC_PAL_MAX_MISMATCH; 2n > TC_MAX_N; a comp with comp[comp[x]] != x for some x.  n = 0: TC_OK, nothing
 * read, 0 palindromes.  The calls take the text only: the joint text S = text . sigma(reverse(text)) of 2n bytes, its
 * enhanced suffix array and all scratch (42 bytes per text byte behind the sort: S 2, its suffix array, inverse suffix
 * array and LCP array 24, the packed centre words 16; the sort's own need behind the first 26 where that is larger) live
 * in the calling ctx's workspace.  The _dev forms take the text and the arrays in HBM; comp, npal and the three words of
 * tc_longest_palindrome stay in host memory. */
#define TC_PAL_MAX_MISMATCH 16
int tc_palindromes(tc_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch, uint32_t min_len,
                   uint32_t *pal_start, uint32_t *pal_len, uint32_t *pal_mm, uint64_t *npal);
int tc_palindromes_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch,
                       uint32_t min_len, uint32_t *d_pal_start, uint32_t *d_pal_len, uint32_t *d_pal_mm, uint64_t *npal);
int tc_longest_palindrome(tc_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch,
                          uint32_t *start, uint32_t *len, uint32_t *mm);
int tc_longest_palindrome_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch,
                              uint32_t *start, uint32_t *len, uint32_t *mm);
/* ---- the minimal absent words of a text (not part of the reference's surface) ----
 * A word x of length >= 2 over bytes is a MINIMAL ABSENT WORD (MAW) of text[0..n) if x does not occur in the text, x
 * without its first byte occurs, and x without its last byte occurs.  Absent single bytes are not reported.  Write
 * x = a . w . b, where w may be empty.
 * N = n + 1 rows, with sa, lcp and left(r) exactly as tc_repeats defines them: row 0 is the empty suffix, left is Nothing
 * for the one row with sa = 0, and left(0) = text[n-1].  IN ROWS: a NODE is the root [0, N-1] with l = 0, or an LCP interval
 * [lb, rb] of depth l as in tc_repeats: lb < rb, l = min lcp[lb+1 .. rb], lcp[lb] < l, rb = N - 1 or lcp[rb+1] < l.  The
 * BOUNDARIES of a node are the rows k in (lb, rb] with lcp[k] = l; its CHILDREN are the maximal row ranges between
 * boundaries.  The child that starts at lb is dropped when sa[lb] + l = n: that suffix is w itself at the end of the text, so
 * it has no next byte.  For a child [cl, cr] whose next byte is b = text[sa[cl] + l], let Lw = the set of bytes left(r) over
 * lb <= r <= rb, without Nothing, and Lc the same over cl <= r <= cr.  The MAWs hanging off this child are a . w . b for
 * every a in Lw \ Lc; their length is l + 2.  A MAW a . w . b exists only where w is empty or a maximal repeat.
 * OUTPUT, one entry per MAW: maw_left = a, maw_pos = sa[cl] (0-based), maw_len = l + 2.  The word is the byte maw_left
 * followed by text[maw_pos .. maw_pos + maw_len - 1).
 * ORDER: every row k >= 1 is a boundary of exactly one node, the one with l = lcp[k].  Row k reports the child [k, q-1]
 * that starts at it, and -- when k is the node's first boundary -- the first child [lb, k-1] before that, unless it is
 * dropped.  The list is in increasing k; within a child, increasing a.  That is deterministic, like the representative-row
 * order of tc_repeats; it is NOT sorted by word.
 *   text          (a, pos, len)                                  words
 *   abaab         (a,2,3) (b,3,3) (a,0,4) (b,4,2)                aaa bab aaba bb
 *   aaabaab       (a,0,4) (b,0,4) (b,1,5) (b,5,3) (b,6,2)        aaaa baaa baaba bab bb
 *   mississippi   18 words: ii mip pip pis missip sissis im mm pm sm mp sp ipi ppp ms ps isi sss
 * A text that holds each of the 256 byte values once has the 65 281 words ab that are not adjacent pairs and nothing
 * longer.  A unary text a^n has the one word a^(n+1): a^n occurs and a^(n+1) does not; so n = 1 has one word, of length 2.
 * FILTERS: only words with min_len <= len, and len <= max_len unless max_len = 0 (no limit), are reported.  min_len < 2, or
 * a max_len that is neither 0 nor >= min_len: TC_ERR_ARG.
 * *nmaw: in = capacity of the three arrays, out = the count.  Too small: TC_ERR_CAPACITY, *nmaw = the needed count, nothing
 * written to the three arrays.  maw_left = maw_pos = maw_len = NULL with capacity 0 is the sizes-only form: TC_OK, the
 * count written.  No simple capacity is always enough -- the count is O(sigma n), at most 512 per row -- so size first.
 * tc_absent_word_profile: hist[len] = the number of MAWs of length len for len <= kmax (kmax + 1 entries, hist[0] =
 * hist[1] = 0), 2 <= kmax <= 4096; *total (may be NULL) = the MAWs of every length.  hist equals the histogram of maw_len of
 * the list call with the window (2, 0).
 * ERRORS AND EDGES.  Null buffers or n > TC_MAX_N: TC_ERR_ARG.  n = 0: TC_OK, 0 words (an all-zero hist), nothing read.
 * The calls take the text only: the suffix array, the LCP array, the last column and all scratch (25 bytes per text byte
 * behind the sort: sa 4, lcp 4, last column 1, the rows' counts 8, the left-context change counts 8, and 36 / (f - 1) for the
 * two trees of fan-out f = 64; the sort's own need where that is larger; the host form of the list adds 9 bytes per slot of
 * capacity) live in the calling ctx's workspace.  The _dev forms take the text and every array (hist included) in HBM; nmaw
 * and total stay host words. */
int tc_absent_words(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t max_len, uint8_t *maw_left,
                    uint32_t *maw_pos, uint32_t *maw_len, uint64_t *nmaw);
int tc_absent_words_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t max_len, uint8_t *d_maw_left,
                        uint32_t *d_maw_pos, uint32_t *d_maw_len, uint64_t *nmaw);
int tc_absent_word_profile(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t kmax, uint64_t *hist, uint64_t *total);
int tc_absent_word_profile_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t kmax, uint64_t *d_hist, uint64_t *total);
/* ---- what is unique in a text: shortest unique prefixes, minimal unique substrings, the shortest unique substring at
 * every position (not part of the reference's surface) ----
 * A substring is UNIQUE when it occurs exactly once in text[0..n).  Occurrences may overlap; the empty string is never
 * unique.  All positions are 0-based, and the end of the text matches nothing.
 * SHORTEST UNIQUE PREFIX: up[i], for 0 <= i < n, is the length of the shortest unique substring that starts at i, and 0
 * where none does -- exactly when the whole suffix at i occurs again as a prefix of another suffix.  IN ROWS, with
 * N = n + 1, sa and lcp as tc_lcp_array defines them and lcp[N] counted as 0: for the row r with sa[r] = i let
 * m = max(lcp[r], lcp[r+1]); then up[i] = m + 1 if i + m < n, else 0.
 * MINIMAL UNIQUE SUBSTRING (MUS): text[s .. s+len) is a MUS when it is unique while it occurs at least twice without its
 * first byte and at least twice without its last byte.  The empty string counts as occurring twice, so a byte that occurs
 * once is a MUS of length 1.  Equivalently, s starts a MUS of length up[s] iff up[s] != 0 and (s = n - 1, or up[s+1] = 0,
 * or up[s+1] >= up[s]).  No MUS contains another, so starts and ends both increase strictly along the list; there are at
 * most n of them, so capacity n is always enough; a non-empty text has at least one.
 * SHORTEST UNIQUE SUBSTRING AT A POSITION (point SUS): for every position p, the shortest unique substring
 * text[s .. s+len) with s <= p < s + len; of equal lengths, the one with the smallest s.  Every unique substring contains a
 * MUS, so with the MUS list (s_k, e_k = s_k + len_k - 1) the answer at p is the best of up to three candidates: the shortest
 * MUS with s_k <= p <= e_k, leftmost on ties, as (s_k, len_k); the MUS with the largest e_k < p, extended right, as
 * (s_k, p - s_k + 1); the MUS with the smallest s_k > p, extended left, as (p, e_k - p + 1).
 *   text          up                      MUS (start, len)                   point SUS (start, len) for p = 0 .. n-1
 *   mississippi   1 5 4 3 5 4 3 2 2 2 0   (0,1) (3,3) (7,2) (8,2) (9,2)      (0,1) (0,2) (0,3) (3,3) (3,3) (3,3) (6,3) (7,2) (7,2) (8,2) (9,2)
 *   abaab         3 2 2 0 0               (1,2) (2,2)                        (0,3) (1,2) (1,2) (2,2) (2,3)
 *   banana        1 4 3 0 0 0             (0,1) (2,3)                        (0,1) (0,2) (0,3) (2,3) (2,3) (2,4)
 *   abcabc        4 3 2 0 0 0             (2,2)                              (0,4) (1,3) (2,2) (2,2) (2,3) (2,4)
 *   aaaa          4 0 0 0                 (0,4)                              (0,4) (0,4) (0,4) (0,4)
 *   a             1                       (0,1)                              (0,1)
 * The MUS of mississippi are m, sis, ip, pp, pi; of abaab ba, aa; of banana b, nan; of abcabc ca.
 * tc_unique_prefixes: up, n entries.
 * tc_unique_substrings: two arrays mus_start = s and mus_len = len, in increasing start.  FILTERS: only MUS with
 * min_len <= len, and len <= max_len unless max_len = 0 (no limit), are reported.  min_len = 0, or a max_len that is neither
 * 0 nor >= min_len: TC_ERR_ARG.
 * *nmus: in = capacity of the two arrays, out = the count.  Too small: TC_ERR_CAPACITY, *nmus = the needed count, nothing
 * written to the two arrays.  mus_start = mus_len = NULL with capacity 0 is the sizes-only form: TC_OK, the count written.
 * tc_shortest_unique: two arrays sus_start = s and sus_len = len, n entries each.  sus_start alone may be NULL; it is then
 * not written.  The filters of the list do not apply.
 * ERRORS AND EDGES.  A null context, a null required buffer or n > TC_MAX_N: TC_ERR_ARG, before a buffer is touched.  n = 0:
 * TC_OK, nothing read or written, 0 MUS.  The calls take the text only: the suffix array, the LCP array and all scratch (sa 4
 * and lcp 4 bytes per text byte, then up 4: 12 for tc_unique_prefixes -- up is the caller's array in the _dev form -- and for
 * the list; the point call adds the MUS lengths 4, the predecessor and successor arrays 8 and 4 / (f - 1) for the min tree of
 * fan-out f = 64: 24; the host forms add their outputs, 8 bytes per slot of capacity or per position; the sort's own need
 * where that is larger) live in the calling ctx's workspace.  The _dev forms take the text and every array in HBM; nmus
 * stays a host word. */
int tc_unique_prefixes(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *up);
int tc_unique_prefixes_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_up);
int tc_unique_substrings(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t max_len, uint32_t *mus_start,
                         uint32_t *mus_len, uint64_t *nmus);
int tc_unique_substrings_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t max_len,
                             uint32_t *d_mus_start, uint32_t *d_mus_len, uint64_t *nmus);
int tc_shortest_unique(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sus_start, uint32_t *sus_len);
int tc_shortest_unique_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_sus_start, uint32_t *d_sus_len);
/* ---- the repeat cover of a text: which bytes are repeated content, as spans, as a mask, and the text without them (not part
 * of the reference's surface) ----
 * text[0..n), positions 0-based, min_len = L >= 1, min_occ = q >= 2, kind TC_COVER_ALL or TC_COVER_LATER.  Occurrences may
 * overlap.  The end of the text matches nothing.
 * SEED: position i with i + L <= n is a seed iff text[i..i+L) occurs at least q times in the text and, for TC_COVER_LATER, i
 * is not its leftmost occurrence.
 * COVER: byte p is covered iff some seed i has i <= p < i + L.  Equivalently, p is covered iff it lies in an occurrence of
 * some substring of length >= L that occurs >= q times (for LATER: in an occurrence that is not that substring's leftmost).
 * For LATER and q = 2 the cover is the union of [i, i + lpf[i]) over the i with lpf[i] >= L, lpf as tc_lpf_array defines it;
 * for ALL and q = 2, i is a seed iff i + L <= n and (up[i] = 0 or up[i] > L), up as tc_unique_prefixes defines it; for any q,
 * i is a seed of kind ALL iff the L-mer of tc_kmers that holds i has occ >= q.
 * SPANS: the maximal runs of covered bytes as (start, len), in increasing start.  Every len >= L, two spans are at least one
 * byte apart, and there are at most (n + 1) / (L + 1) of them: capacity n is always enough.  covered = the sum of the span
 * lengths.
 * MASK: with a 256-byte map, out[p] = map[text[p]] where p is covered and text[p] elsewhere; with map = NULL, out[p] = 1 / 0,
 * the cover itself as bytes.  n bytes.
 * DEDUP: out is the text with the covered bytes removed, in order: n - covered bytes.  With LATER every string of >= L bytes
 * that occurred earlier is cut out and its first copy kept; with ALL only the content that occurs fewer than q times at
 * length L remains.  The result may hold new repeats across the cuts: what stood left and right of a cut is adjacent now.
 *   text                        L q  kind   spans (start,len)   covered  mask                       dedup
 *   mississippi                 2 2  ALL    (1,7)               7        mISSISSIppi                mppi
 *   mississippi                 2 2  LATER  (4,4)               4        missISSIppi                missppi
 *   mississippi                 1 4  ALL    (1,7) (10,1)        8        mISSISSIppI                mpp
 *   mississippi                 1 4  LATER  (3,5) (10,1)        6        misSISSIppI                mispp
 *   abcabcabc                   3 3  ALL    (0,9)               9        ABCABCABC                  (empty)
 *   abcabcabc                   3 2  LATER  (3,6)               6        abcABCABC                  abc
 *   banana                      2 2  LATER  (3,3)               3        banANA                     ban
 *   aaaa                        2 2  LATER  (1,3)               3        aAAA                       a
 *   abcdabxcd                   2 2  ALL    (0,6) (7,2)         8        ABCDABxCD                  x
 *   abcdabxcd                   2 2  LATER  (4,2) (7,2)         4        abcdABxCD                  abcdx
 *   "the cat sat; the cat ran"  4 2  LATER  (13,8)              8        the cat sat; THE CAT ran   "the cat sat; ran"
 * (masks shown with the map that turns a letter into upper case.)
 * THE GENERAL FORM, tc_cover_*_dev, over an array len of n words in HBM: position i counts iff len[i] >= L, and covers
 * [i, min(n, i + len[i])), the sum taken in 64 bits.  Spans, mask and dedup are defined as above.  The values are compared
 * and added and never used as an index, so the calls stay in bounds on any contents.  With len = lpf it is the LATER cover at
 * q = 2; with len = ms_len of tc_text_match_stats_dev it is the part of a query that is found in a target.
 * CAPACITY.  *nspans and *nout: in = capacity (of the two arrays, of out), out = the count.  Too small: TC_ERR_CAPACITY, the
 * needed count written, nothing written to the arrays.  NULL arrays with capacity 0 is the sizes-only form: TC_OK, the count
 * written.  covered is written in every form where the cover was computed; it may be NULL.
 * ERRORS AND EDGES.  TC_ERR_ARG, before a buffer is touched, for: a null context or required buffer; n > TC_MAX_N;
 * min_len = 0; min_occ < 2; an unknown kind; out overlapping the text; a NULL d_text with a non-NULL map.  n = 0 or
 * min_len > n (the text calls): TC_OK, 0 spans, covered 0, nothing sorted; the mask is the text (zeroes without a map), the
 * dedup is the text.  The text calls take the text only: the suffix array, the LCP array and all scratch (sa 4 and lcp 4
 * bytes per text byte, then len 4, and 4 / (f - 1) for each min tree of fan-out f = 64 -- none for ALL with q = 2, that of
 * lcp for q > 2, that of sa as well for LATER: 12 bytes per text byte and a little; the host forms add their outputs; the
 * sort's own need where that is larger) live in the calling ctx's workspace; the general form needs 36 bytes per 2048
 * positions.  The _dev forms take the text and every array in HBM; map, the counts and covered stay in host memory. */
#define TC_COVER_ALL 0
#define TC_COVER_LATER 1
int tc_repeat_spans(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind,
                    uint32_t *span_start, uint32_t *span_len, uint64_t *nspans, uint64_t *covered);
int tc_repeat_spans_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind,
                        uint32_t *d_span_start, uint32_t *d_span_len, uint64_t *nspans, uint64_t *covered);
int tc_repeat_mask(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind,
                   const uint8_t *map, uint8_t *out, uint64_t *covered);
int tc_repeat_mask_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind,
                       const uint8_t *map, uint8_t *d_out, uint64_t *covered);
int tc_repeat_dedup(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind, uint8_t *out,
                    uint64_t *nout, uint64_t *covered);
int tc_repeat_dedup_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind,
                        uint8_t *d_out, uint64_t *nout, uint64_t *covered);
int tc_cover_spans_dev(tc_ctx *ctx, const uint32_t *d_len, uint64_t n, uint32_t min_len, uint32_t *d_span_start,
                       uint32_t *d_span_len, uint64_t *nspans, uint64_t *covered);
int tc_cover_mask_dev(tc_ctx *ctx, const uint32_t *d_len, const uint8_t *d_text, uint64_t n, uint32_t min_len, const uint8_t *map,
                      uint8_t *d_out, uint64_t *covered);
int tc_cover_dedup_dev(tc_ctx *ctx, const uint32_t *d_len, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint8_t *d_out,
                       uint64_t *nout, uint64_t *covered);
/* ---- a kept enhanced suffix array: build once, batched substring queries (not part of the reference's surface) ----
 * tc_esa is an opaque handle, owned like tc_fm: its own device blocks, not the workspace of the ctx that built it.  It lives
 * until tc_esa_free and is read-only after the build.  WHAT THE HANDLE KEEPS: a copy of the text (n bytes and 16 of padding);
 * sa, lcp and isa, N = n + 1 entries each, sa and lcp exactly as tc_suffix_array_dev and tc_lcp_array_dev define them (row 0
 * is the empty suffix), isa[sa[r]] = r; the min tree over lcp and a min tree over sa, fan-out 64: about 13.2 bytes per text
 * byte in all, tc_esa_device_bytes reports the real figures (part 0 all, 1 text, 2 sa, 3 isa, 4 lcp + its min tree, 5 the min
 * tree of sa; parts 1 .. 5 sum to part 0).  The build sorts and makes the LCP array in the ctx's workspace, which holds scratch
 * only.  n = 0 builds the one-row ESA.  A failed build releases everything and leaves *out NULL.
 * tc_esa_arrays: the device pointers (each out-pointer may be NULL); they stay valid until tc_esa_free and may be passed to
 * tc_kmers_esa_dev, tc_kmer_spectrum_esa_dev, tc_kmer_profile_esa_dev and tc_cover_*_dev: the sort is paid once.
 * tc_esa_read: entries [first, first + count) of one array (what: 1 text, 2 sa, 3 isa, 4 lcp) to host memory, or to device
 * memory with dst_on_device != 0.  A range past the array is TC_ERR_ARG.
 * THE QUERIES, each over nq queries; in the _dev forms every array is in HBM and nq is a host word.  nq = 0: TC_OK, nothing
 * touched.  Positions are 0-based and run 0 .. n inclusive; position n is the empty suffix.  Occurrences may overlap.  The end
 * of the text matches nothing.
 * LCE: len[q] is the largest L with a[q] + L <= n, b[q] + L <= n and at most max_mismatch positions k < L where
 * text[a + k] != text[b + k]; mm[q] is the number of such positions (mm may be NULL).  max_mismatch <= TC_ESA_MAX_MISMATCH.
 * a == b gives n - a and 0 mismatches.
 *   mississippi: (1, 4) gives 4 at max_mismatch 0, 5 with mm = 1 at 1, 7 with mm = 2 at 2; (0, 0) gives 11; (3, 11) gives 0
 * FIND: for the substring text[start .. start + len), first_row[q] is the smallest row whose suffix has the substring as a
 * prefix, occ[q] is the number of such rows, first_pos[q] is the smallest text position where it occurs.  Each of the three
 * may be NULL, but not all three.  len = 0 answers (0, n + 1, 0).
 *   mississippi: (1, 4) "issi" gives first_row 3, occ 2, first_pos 1; (2, 1) "s" gives first_row 8, occ 4, first_pos 2
 * COMPARE: order[q] = -1, 0, 1 as text[a_start .. a_start + a_len) sorts before, equals, sorts behind
 * text[b_start .. b_start + b_len), bytes compared as unsigned; a proper prefix sorts first.  common[q] is the length of
 * their common prefix (common may be NULL).
 *   mississippi: (1, 4) against (4, 4) gives 0, common 4; (1, 4) against (4, 3) gives 1, common 3; (8, 2) against (5, 2) gives
 *   -1, common 0
 * ERRORS.  TC_ERR_ARG for: a null context, handle or required buffer; max_mismatch > TC_ESA_MAX_MISMATCH; n > TC_MAX_N; a
 * handle built on another device than the ctx's; a query that leaves the text (a position above n, start + len > n) in both
 * forms -- the kernel raises a flag, every access stays in bounds, and the outputs of the batch are unspecified.  Any number
 * of ctxs on the handle's device may query one handle at the same time; in the calling ctx's workspace a query batch needs
 * its flag word and, in the host form, the bytes of its arrays. */
typedef struct tc_esa tc_esa;
#define TC_ESA_MAX_MISMATCH 16
int tc_esa_build(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_esa **out);
int tc_esa_build_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_esa **out);
void tc_esa_free(tc_esa *esa);
uint64_t tc_esa_n(const tc_esa *esa);
uint64_t tc_esa_device_bytes(const tc_esa *esa, int part);
int tc_esa_arrays(const tc_esa *esa, const uint8_t **d_text, const uint32_t **d_sa, const uint32_t **d_lcp, const uint32_t **d_isa);
int tc_esa_read(tc_ctx *ctx, const tc_esa *esa, int what, uint64_t first, uint64_t count, void *dst, int dst_on_device);
int tc_esa_lce(tc_ctx *ctx, const tc_esa *esa, const uint32_t *a, const uint32_t *b, uint64_t nq, uint32_t max_mismatch,
               uint32_t *len, uint32_t *mm);
int tc_esa_lce_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_a, const uint32_t *d_b, uint64_t nq, uint32_t max_mismatch,
                   uint32_t *d_len, uint32_t *d_mm);
int tc_esa_find(tc_ctx *ctx, const tc_esa *esa, const uint32_t *start, const uint32_t *len, uint64_t nq, uint32_t *first_row,
                uint32_t *occ, uint32_t *first_pos);
int tc_esa_find_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_start, const uint32_t *d_len, uint64_t nq,
                    uint32_t *d_first_row, uint32_t *d_occ, uint32_t *d_first_pos);
int tc_esa_compare(tc_ctx *ctx, const tc_esa *esa, const uint32_t *a_start, const uint32_t *a_len, const uint32_t *b_start,
                   const uint32_t *b_len, uint64_t nq, int8_t *order, uint32_t *common);
int tc_esa_compare_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_a_start, const uint32_t *d_a_len,
                       const uint32_t *d_b_start, const uint32_t *d_b_len, uint64_t nq, int8_t *d_order, uint32_t *d_common);
/* ---- document collections on the kept ESA: document frequency and listing (not part of the reference's surface) ----
 * The text is the concatenation of ndocs documents WITHOUT separators; doc_start[0 .. ndocs] (host memory in both forms) gives
 * the boundaries: doc_start[0] = 0, non-decreasing, doc_start[ndocs] = n.  Empty documents are allowed.  1 <= ndocs <=
 * TC_ESA_MAX_DOCS.  THE FIRST-BYTE RULE: an occurrence belongs to the document that holds its first byte, so an occurrence that
 * runs across a boundary counts for the document it starts in.  A caller who must not see such matches puts a byte between the
 * documents that their queries do not contain.  All 256 byte values stay legal in the text.
 * tc_esa_build_docs / _dev: the handle of tc_esa_build and, over its N = n + 1 rows, da[r] = the document of sa[r]
 * (TC_ESA_NO_DOC for row 0, the empty suffix), pv[r] = 1 + the largest row r' < r with da[r'] = da[r], 0 where there is none
 * (pv[0] = 0xffffffff), and a min tree over pv: 8 bytes per text byte and one tree more, about 21.2 in all.  A doc_start that
 * breaks the rules is TC_ERR_ARG before any device work.  n = 0 with all documents empty builds the one-row handle.  A failed build
 * releases everything and leaves *out NULL.  Every query and analysis of a plain handle works on a handle with documents
 * unchanged.  tc_esa_ndocs: 0 for a plain handle.  tc_esa_doc_arrays: the device pointers (each out-pointer may be NULL), valid
 * until tc_esa_free.  tc_esa_read takes what = 5 (da), 6 (pv), 7 (doc_start, ndocs + 1 entries); tc_esa_device_bytes part 6 (da +
 * doc_start) and part 7 (pv + its min tree), 0 on a plain handle; on every handle parts 1 .. 7 sum to part 0.
 * THE QUERIES are over substrings text[start .. start + len) as tc_esa_find takes them.  On a plain handle: TC_ERR_ARG.
 * DOC COUNT: df[q] is the number of distinct documents with an occurrence; with limit > 0 the count saturates at limit (limit 2
 * asks "in more than one document?"), limit 0 counts all.  occ[q] is the number of occurrences as in tc_esa_find (occ may be
 * NULL).  len = 0 counts the non-empty documents.
 * DOC LIST: the documents of query q are docs[list_offs[q] .. list_offs[q + 1]), in the order of their first row in the
 * substring's suffix-array interval; hit_pos (may be NULL) is sa of that row: one occurrence in that document.  At most limit
 * documents per query when limit > 0.  list_offs has nq + 1 entries.  *ntotal: in = capacity of docs and hit_pos, out = the
 * total; too small: TC_ERR_CAPACITY, *ntotal = the needed total, nothing written to docs or hit_pos (capacity 0 with NULL arrays
 * asks for the sizes).  A sizes pass and a fill pass without atomics: two calls give identical output.
 *   banana . bandana . ananas, doc_start = {0, 6, 13, 19}: (1, 3) "ana" has 5 occurrences in documents 1, 0, 2 with hit_pos 10,
 *   3, 13; (0, 3) "ban" is in documents 0, 1; (2, 3) "nan" in 0, 2; (9, 1) "d" in 1; (3, 4) "anab" in 0 -- it starts in banana
 *   and ends in bandana: the first-byte rule; (0, 0) lists every non-empty document: 1, 0, 2
 * K-MER DOCS: the k-mers of tc_kmers_esa_dev with no occurrence filter, in the same order and with the same kmer_pos, kmer_occ
 * and kmer_row, and kmer_df, the number of distinct documents a k-mer occurs in; filtered to min_df <= df, and df <= max_df unless
 * max_df = 0 (no upper bound): (1, 1) lists the markers of a single document, (ndocs, 0) the k-mers every document has.  Each
 * output may be NULL.  *nk: in = capacity of the arrays, out = the count; too small: TC_ERR_CAPACITY, *nk = the needed count,
 * nothing written (capacity 0 with all arrays NULL asks for the count).  k = 0 is TC_ERR_ARG, k > n gives no k-mer.
 * K-MER DOC SPECTRUM: hist[d], d = 0 .. ndocs, is the number of distinct k-mers that occur in exactly d documents (the core /
 * shell / cloud curve; hist[0] is 0), *distinct their number: the hist sum to it.  hist is host memory, d_hist device memory.
 *   the example above, k = 3: 11 distinct 3-mers, eight in one document, "ban" and "nan" in two, "ana" in all three (occ 5): hist
 *   = {0, 8, 2, 1}
 * ERRORS as for the queries above: a query that leaves the text is TC_ERR_ARG in both forms -- the kernel raises a flag, every
 * access stays in bounds; nq = 0: TC_OK, nothing touched. */
#define TC_ESA_MAX_DOCS 65535
#define TC_ESA_NO_DOC 0xffffffffu
int tc_esa_build_docs(tc_ctx *ctx, const uint8_t *text, uint64_t n, const uint32_t *doc_start, uint32_t ndocs, tc_esa **out);
int tc_esa_build_docs_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint32_t *doc_start, uint32_t ndocs, tc_esa **out);
uint32_t tc_esa_ndocs(const tc_esa *esa);
int tc_esa_doc_arrays(const tc_esa *esa, const uint32_t **d_doc_start, const uint32_t **d_da, const uint32_t **d_pv);
int tc_esa_doc_count(tc_ctx *ctx, const tc_esa *esa, const uint32_t *start, const uint32_t *len, uint64_t nq, uint32_t limit,
                     uint32_t *df, uint32_t *occ);
int tc_esa_doc_count_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_start, const uint32_t *d_len, uint64_t nq, uint32_t limit,
                         uint32_t *d_df, uint32_t *d_occ);
int tc_esa_doc_list(tc_ctx *ctx, const tc_esa *esa, const uint32_t *start, const uint32_t *len, uint64_t nq, uint32_t limit,
                    uint64_t *list_offs, uint32_t *docs, uint32_t *hit_pos, uint64_t *ntotal);
int tc_esa_doc_list_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_start, const uint32_t *d_len, uint64_t nq, uint32_t limit,
                        uint64_t *d_list_offs, uint32_t *d_docs, uint32_t *d_hit_pos, uint64_t *ntotal);
int tc_esa_kmer_docs(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint32_t min_df, uint32_t max_df, uint32_t *kmer_pos,
                     uint32_t *kmer_occ, uint32_t *kmer_df, uint32_t *kmer_row, uint64_t *nk);
int tc_esa_kmer_docs_dev(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint32_t min_df, uint32_t max_df, uint32_t *d_kmer_pos,
                         uint32_t *d_kmer_occ, uint32_t *d_kmer_df, uint32_t *d_kmer_row, uint64_t *nk);
int tc_esa_kmer_doc_spectrum(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint64_t *hist, uint64_t *distinct);
int tc_esa_kmer_doc_spectrum_dev(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint64_t *d_hist, uint64_t *distinct);
/* ---- cross-document matches on the kept ESA: per position and per document (not part of the reference's surface) ----
 * Which parts of each document also occur in another document, how long are those matches, and where is the other copy?  The
 * handle is one of tc_esa_build_docs: the text of n bytes, doc_start[0 .. ndocs] and the first-byte rule above.  The document of
 * position i is d(i).  A position j QUALIFIES for i under kind: TC_DOC_OTHER (0): d(j) != d(i); TC_DOC_EARLIER (1): d(j) < d(i).
 * PER POSITION (tc_esa_doc_match): among the qualifying suffixes take the lexicographic predecessor a and the successor b of
 * suffix i; either may be missing.  La and Lb are their common-prefix lengths with suffix i in the concatenated text, -1 where
 * missing.  L = max(La, Lb); the partner is a if La >= Lb, else b.  If L <= 0: xl[i] = 0, src[i] = TC_ESA_NO_POS, xdoc[i] =
 * TC_ESA_NO_DOC.  Otherwise src[i] = the partner's position and xdoc[i] = its document, and xl[i] = L, or with clamp != 0 it is
 * min(L, doc_start[d(i) + 1] - i).  The clamp is on i's own side only; the partner's side follows the first-byte rule.  In row
 * terms, r = isa[i]: a and b are the nearest qualifying rows >= 1 above and below r, La and Lb the range minima of lcp over
 * (a, r] and (r, b]; row 0, the empty suffix, never qualifies.  With clamp = 0, for TC_DOC_OTHER xl[i] >= L iff
 * tc_esa_doc_count of (i, L) at limit 2 answers 2; for TC_DOC_EARLIER iff the document list of (i, L) holds a document below
 * d(i).  Each output has n entries and may be NULL; all NULL is TC_ERR_ARG.  xl is what tc_cover_spans_dev, tc_cover_mask_dev and
 * tc_cover_dedup_dev take: with TC_DOC_OTHER they mask or remove what a document shares with the others, with TC_DOC_EARLIER the
 * first copy of everything stays.
 * PER DOCUMENT (tc_esa_doc_shared), always clamped: shared[d] is the number of bytes p of document d for which some i <= p in d
 * has clamped xl[i] >= min_len and p < i + xl[i]; shared[d] over the size of d is the containment of d in the rest (or in the
 * earlier part) of the collection.  longest[d] is the maximum clamped xl over d's positions, 0 for an empty document; it does not
 * depend on min_len.  ndocs entries each; either may be NULL, both NULL is TC_ERR_ARG.
 * ERRORS: TC_ERR_ARG before any device work for a null context or handle, a plain handle (tc_esa_ndocs 0), a kind other than the
 * two, min_len = 0.  n = 0 is TC_OK with nothing touched for match, and zeros for shared.  One document gives all-zero xl, src =
 * TC_ESA_NO_POS and zero shared for both kinds.  Two calls give identical output.  The handle is read-only: all scratch is the
 * calling context's workspace, so two contexts may query one handle at once.
 *   example 1: banana . bandana . ananas, doc_start = {0, 6, 13, 19}, TC_DOC_OTHER (the clamp changes nothing here):
 *     xl = 3 5 4 3 2 1 3 2 1 0 3 2 1 5 4 3 2 1 0
 *     src = 6 13 14 10 11 12 0 15 16 - 3 4 5 1 2 1 2 7 -
 *     xdoc = 1 2 2 1 1 1 0 2 2 - 0 0 0 0 0 0 0 1 -
 *     shared at min_len 1, 2, 3 alike = {6, 6, 5}, longest = {5, 3, 5}: only the d of bandana and the last s are private
 *   example 2: the same collection, TC_DOC_EARLIER:
 *     xl = 0 0 0 0 0 0 3 2 1 0 3 2 1 5 4 3 2 1 0
 *     src = - - - - - - 0 1 2 - 3 4 5 1 2 1 2 7 -
 *     shared = {0, 6, 5}, longest = {0, 3, 5}
 *   example 3: ab . cab . abc, doc_start = {0, 2, 5, 8}, TC_DOC_OTHER: position 0 matches abc at 5 across its own end:
 *     unclamped xl = 3 2 1 2 1 3 2 1
 *     xl = 2 1 1 2 1 3 2 1
 *     src = 5 6 7 5 6 0 1 2
 *     xdoc = 2 2 2 2 2 0 0 1
 *     shared at min_len 1 / 2 / 3 = {2, 3, 3} / {2, 2, 3} / {0, 0, 3}, longest = {2, 2, 3}; at min_len 2 the cover is 1 1 0 1 1 1 1
 *     1: spans (0, 2) and (3, 5), and the dedup leaves c
 *   example 4: the same collection, TC_DOC_EARLIER:
 *     xl = 0 0 0 2 1 3 2 1
 *     src = - - - 0 1 0 1 2
 *     xdoc = - - - 0 0 0 0 1
 *     at min_len 2 the cover is 0 0 0 1 1 1 1 1 and the dedup leaves abc: the first copy of everything stays */
#define TC_DOC_OTHER 0
#define TC_DOC_EARLIER 1
#define TC_ESA_NO_POS 0xffffffffu
int tc_esa_doc_match(tc_ctx *ctx, const tc_esa *esa, int kind, int clamp, uint32_t *xl, uint32_t *src, uint32_t *xdoc);
int tc_esa_doc_match_dev(tc_ctx *ctx, const tc_esa *esa, int kind, int clamp, uint32_t *d_xl, uint32_t *d_src, uint32_t *d_xdoc);
int tc_esa_doc_shared(tc_ctx *ctx, const tc_esa *esa, int kind, uint32_t min_len, uint64_t *shared, uint32_t *longest);
int tc_esa_doc_shared_dev(tc_ctx *ctx, const tc_esa *esa, int kind, uint32_t min_len, uint64_t *d_shared, uint32_t *d_longest);
/* ---- the k-mers of a text: list, abundance spectrum and all-k profile (not part of the reference's surface) ----
 * N = n + 1 rows; sa and lcp as tc_lcp_array defines them (row 0 is the empty suffix, the end of the text matches
 * nothing); lcp[0] counts as 0 whatever the array holds, and lcp[N] as 0.  For k >= 1 row q is a BOUNDARY iff lcp[q] < k;
 * row N is a boundary too.  A K-MER is the row interval [p, q) between two consecutive boundaries whose first row is long
 * enough, sa[p] + k <= n (the rows p+1 .. q-1 have lcp >= k, so they are long enough as well; a suffix shorter than k is
 * always a boundary and never a member).  kmer_occ = q - p, kmer_pos = sa[p] (0-based: the occurrence whose suffix sorts
 * first), kmer_row = p; all occurrences are sa[row .. row + occ).  ORDER: increasing row, the lexicographic order of the
 * k-mers; every k-mer appears once.  FILTERS: min_occ <= occ, and occ <= max_occ unless max_occ = 0 (no upper bound):
 * (1, 0) lists all k-mers, (1, 1) the unique ones, (2, 0) the repeated ones.  Over all k-mers the occ sum to
 * max(0, n - k + 1); k > n: no k-mers.  k = 0, min_occ = 0, or max_occ non-zero and below min_occ: TC_ERR_ARG.
 *   "mississippi", k = 2: sa = 11 10 7 4 1 0 9 8 6 3 5 2, lcp = 0 0 1 1 4 0 0 1 0 2 1 3, and (row, pos, occ) =
 *       (2,7,1) (3,4,2) (5,0,1) (6,9,1) (7,8,1) (8,6,2) (10,5,2): ip, is x2, mi, pi, pp, si x2, ss x2
 *   "aaabaab": sa = 7 0 4 1 5 2 6 3, lcp = 0 0 2 3 1 2 0 1; k = 2: (1,0,3) (4,5,2) (7,3,1); k = 1: (1,0,5) (6,6,2)
 *   "aaaaaa", k = 2: (2,4,5)
 * *nk: in = capacity of the three arrays, out = the count.  Too small: TC_ERR_CAPACITY, *nk = the needed count, nothing
 * written to the three arrays.  kmer_pos = kmer_occ = NULL with capacity 0 is the sizes-only form: TC_OK, the count
 * written.  Capacity n is always enough.  sa (n + 1 entries) and kmer_row may each be NULL.
 * THE SPECTRUM, for bins in 1 .. 65536 (anything else: TC_ERR_ARG): hist[i] for i < bins - 1 = the number of distinct
 * k-mers with occ = i + 1, hist[bins - 1] = the number with occ >= bins; *distinct = the sum of hist,
 * *total = max(0, n - k + 1).  No filters.  d_hist (bins words, in HBM) is zeroed by the call.
 * THE PROFILE, for kmax in 1 .. 4096 (anything else: TC_ERR_ARG) and every k = 1 .. kmax: distinct[k-1] = the number of
 * distinct k-mers = max(0, n-k+1) - #{r : lcp[r] >= k}, unique[k-1] = the number of k-mers with occ = 1 =
 * #{r in 1 .. n : max(lcp[r], lcp[r+1]) < k} - min(k-1, n).  unique may be NULL.  Both are HOST arrays in every form, as
 * *nk, *distinct and *total are host words.
 * ERRORS AND EDGES.  Null buffers, n > TC_MAX_N, N = 0 or N - 1 > TC_MAX_N: TC_ERR_ARG.  n = 0: TC_OK, 0 k-mers, all-zero
 * hist and profile; sa, when given, receives its one entry 0.
 * The text forms build the enhanced suffix array in the calling ctx's workspace (8 bytes per text byte behind the sort:
 * sa 4, lcp 4; the sort's own need where that is larger; tc_kmers_dev sorts straight into a d_sa the caller gives) and then
 * do what the _esa_dev forms do.  THE _esa_dev FORMS take arrays the caller kept from tc_suffix_array_dev and
 * tc_lcp_array_dev -- the sort is paid once for any number of k.  They stay in bounds on ANY contents: boundaries come from
 * the d_lcp values alone, d_sa values are copied and compared (in 64 bits) and never used as an index; arrays that are not
 * an enhanced suffix array give values without meaning, and no error.  The profile never reads sa.
 * Scratch behind the arrays, from the calling ctx's workspace: 8 bytes per tile of 4096 rows (the tiles' last boundaries
 * and carries), 16 per tile and the scan's sums for the list, 2 (kmax + 1) words for the profile.  Nothing per row.
 * Cost: the list is two passes over lcp (count, fill) behind one for the tiles' boundaries, one read of sa per group and
 * the stores; the spectrum two passes over lcp and one read of sa per group; the profile one pass over lcp. */
int tc_kmers(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ, uint32_t *sa,
             uint32_t *kmer_pos, uint32_t *kmer_occ, uint32_t *kmer_row, uint64_t *nk);
int tc_kmers_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ, uint32_t *d_sa,
                 uint32_t *d_kmer_pos, uint32_t *d_kmer_occ, uint32_t *d_kmer_row, uint64_t *nk);
int tc_kmers_esa_dev(tc_ctx *ctx, const uint32_t *d_sa, const uint32_t *d_lcp, uint64_t N, uint32_t k, uint32_t min_occ,
                     uint32_t max_occ, uint32_t *d_kmer_pos, uint32_t *d_kmer_occ, uint32_t *d_kmer_row, uint64_t *nk);
int tc_kmer_spectrum(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t k, uint32_t bins, uint64_t *hist, uint64_t *distinct,
                     uint64_t *total);
int tc_kmer_spectrum_esa_dev(tc_ctx *ctx, const uint32_t *d_sa, const uint32_t *d_lcp, uint64_t N, uint32_t k, uint32_t bins,
                             uint64_t *d_hist, uint64_t *distinct, uint64_t *total);
int tc_kmer_profile(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t kmax, uint64_t *distinct, uint64_t *unique);
int tc_kmer_profile_esa_dev(tc_ctx *ctx, const uint32_t *d_lcp, uint64_t N, uint32_t kmax, uint64_t *distinct, uint64_t *unique);
/* ---- one text against another: matching statistics, maximal exact matches, longest common substring (not part of the
 * reference's surface) ----
 * Q is the query (a bytes), T the target (b bytes), a + b <= TC_MAX_N; all positions 0-based.  For every 0 <= i < a:
 *   ms_len[i] = the largest l such that Q[i .. i+l) occurs in T.  The match lies inside both texts and never runs over an
 *               end; l = 0: the byte Q[i] does not occur in T.
 *   ms_pos[i] = the start in T of the lexicographically smallest suffix of T that has that string as a prefix (the end of
 *               the text sorts first, as everywhere here); 0 where l = 0.
 *   ms_occ[i] = the number of occurrences of that string in T, overlapping ones included; 0 where l = 0.
 * (ms_len, ms_pos + 1, ms_occ) is what tc_fm_match_stats answers for the single pattern Q on an index of T built by
 * tc_fm_build_lcp.  ms_pos and ms_occ may each be NULL; ms_len may not.
 * THE MEMS for min_len >= 1 are the triples (mem_start, mem_pos, mem_len) = (i, ms_pos[i], ms_len[i]) with
 * ms_len[i] >= min_len and (i = 0 or ms_len[i-1] <= ms_len[i]), in increasing i: the rule of tc_fm_mems.  *nmem (a host
 * word): in = capacity of the three arrays, out = the count.  Too small: TC_ERR_CAPACITY, *nmem = the needed count, nothing
 * written to the arrays.  mem_start = mem_pos = mem_len = NULL with capacity 0 is the sizes-only form: TC_OK, the count
 * written.  Capacity a is always enough.  tc_mems_from_stats_dev is the filter alone over two arrays of a entries in HBM,
 * so that one tc_text_match_stats_dev serves any number of min_len; it compares and copies the array values and never
 * uses one as an index, so it stays in bounds on any contents (d_ms_pos may be NULL in its sizes-only form).
 * THE LCS: *len = the largest ms_len, *qpos = the smallest i that attains it, *tpos = ms_pos[qpos] -- Q[qpos .. qpos+len)
 * = T[tpos .. tpos+len) is a longest common substring -- and (0, 0, 0) when no byte is common; *sum = the sum of ms_len
 * (sum / a, the mean matching-statistics length, is the usual similarity estimate).  The four are host words in both forms.
 *     Q         T         ms_len        ms_pos        ms_occ        MEMs at min_len 1         LCS (len, qpos, tpos), sum
 *     "banana"  "ananas"  0 5 4 3 2 1   0 0 1 0 1 0   0 1 1 2 2 3   (1,0,5)                   (5, 1, 0), 15
 *     "ab"      "abab"    2 1           2 3           2 2           (0,2,2)                   (2, 0, 2), 3
 *     "aaaaa"   "aaa"     3 3 3 2 1     0 0 0 1 2     1 1 1 2 3     (0,0,3) (1,0,3) (2,0,3)   (3, 0, 0), 12
 * ERRORS AND EDGES.  A NULL required buffer, a + b > TC_MAX_N or min_len = 0: TC_ERR_ARG, nothing written.  a = 0: TC_OK,
 * nothing read or written, 0 MEMs, an LCS of all zeros.  b = 0: zeros to every given array, 0 MEMs, no sort.  Q and T may
 * be the same buffer or overlap (both are only read): for Q = T, ms_len[i] = a - i.
 * The calls take the two texts only.  They are copied into one text Q T whose enhanced suffix array answers everything;
 * that text, the arrays and all scratch (25 bytes per byte of the two texts behind the sort: the text 1, sa 4, lcp 4, the
 * T-row flags and then the two row lists 8, the T-row counts 8; up to 12 bytes per query byte for results the caller did
 * not give in HBM; the sort's own need where that is larger) live in the calling ctx's workspace.  The _dev forms take the
 * two texts as separate HBM pointers and every array in HBM. */
int tc_text_match_stats(tc_ctx *ctx, const uint8_t *query, uint64_t a, const uint8_t *target, uint64_t b, uint32_t *ms_len,
                        uint32_t *ms_pos, uint32_t *ms_occ);
int tc_text_match_stats_dev(tc_ctx *ctx, const uint8_t *d_query, uint64_t a, const uint8_t *d_target, uint64_t b,
                            uint32_t *d_ms_len, uint32_t *d_ms_pos, uint32_t *d_ms_occ);
int tc_text_mems(tc_ctx *ctx, const uint8_t *query, uint64_t a, const uint8_t *target, uint64_t b, uint32_t min_len,
                 uint32_t *mem_start, uint32_t *mem_pos, uint32_t *mem_len, uint64_t *nmem);
int tc_text_mems_dev(tc_ctx *ctx, const uint8_t *d_query, uint64_t a, const uint8_t *d_target, uint64_t b, uint32_t min_len,
                     uint32_t *d_mem_start, uint32_t *d_mem_pos, uint32_t *d_mem_len, uint64_t *nmem);
int tc_text_lcs(tc_ctx *ctx, const uint8_t *query, uint64_t a, const uint8_t *target, uint64_t b, uint32_t *len, uint64_t *qpos,
                uint64_t *tpos, uint64_t *sum);
int tc_text_lcs_dev(tc_ctx *ctx, const uint8_t *d_query, uint64_t a, const uint8_t *d_target, uint64_t b, uint32_t *len,
                    uint64_t *qpos, uint64_t *tpos, uint64_t *sum);
int tc_mems_from_stats_dev(tc_ctx *ctx, const uint32_t *d_ms_len, const uint32_t *d_ms_pos, uint64_t a, uint32_t min_len,
                           uint32_t *d_mem_start, uint32_t *d_mem_pos, uint32_t *d_mem_len, uint64_t *nmem);

/* bytestringFromWord8BWT (BWT.hs:108-110) = fromBWT (:93-104) + sortTB
 * (BWT/Internal.hs:144-149) + magicInverseBWT (:163-200), for a well-formed BWT
 * (exactly one Nothing at `primary`).  text receives N-1 bytes. */
int tc_bwt_decode(tc_ctx *ctx, const uint8_t *L, uint64_t N, uint64_t primary, uint8_t *text);
/* The same for ANY Seq (Maybe Word8) (zero or several Nothings):
 * n_out = bytes produced (<= N); TC_ERR_MALFORMED where fromJust would throw. */
int tc_bwt_decode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint8_t *text,
                      uint64_t *n_out);

/* ---- Data.MTF ------------------------------------------------------------ */
/* bytestringBWTToMTFB (MTF.hs:117-122) = seqToMTF (MTF/Internal.hs:128-175):
 * idx[N] 0-based list positions; final_list[sigma] = list AFTER the last move;
 * alphabet = sorted present symbols, Nothing first.  primary < 0: no Nothing. */
int tc_mtf_encode(tc_ctx *ctx, const uint8_t *L, uint64_t N, int64_t primary, uint16_t *idx,
                  int16_t *final_list, uint32_t *sigma);
/* bytestringToMTFB-shaped input (MTF.hs:157-161): any Seq (Maybe Word8). */
int tc_mtf_encode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint16_t *idx,
                      int16_t *final_list, uint32_t *sigma);
/* bytestringBWTFromMTFB (MTF.hs:240-245) = seqFromMTF (MTF/Internal.hs:201-232):
 * initial list = sort(unique(list)) (:214); out-of-range index => TC_ERR_MALFORMED
 * (DS.index).  N == 0 or nlist == 0 => empty output (:202-209). */
int tc_mtf_decode(tc_ctx *ctx, const uint16_t *idx, uint64_t N, const int16_t *list,
                  uint32_t nlist, int16_t *sym);

/* ---- Data.RLE ------------------------------------------------------------ */
/* bytestringBWTToRLEB (RLE.hs:117-123) = seqToRLE (RLE/Internal.hs:104-153) incl.
 * the sentinel quirks.  Pair k = (counts[k], syms[k]); the Haskell
 * side renders counts with `show` (RLE/Internal.hs:128).  nruns: in capacity
 * (2N is always enough), out pairs written. */
int tc_rle_encode(tc_ctx *ctx, const uint8_t *L, uint64_t N, int64_t primary, uint32_t *counts,
                  int16_t *syms, uint64_t *nruns);
/* bytestringToRLEB-shaped input (RLE.hs:155-159): any Seq (Maybe Word8). */
int tc_rle_encode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint32_t *counts,
                      int16_t *syms, uint64_t *nruns);
/* Q4b glue: runs of a plain integer stream (the MTF indices; no sentinel). */
int tc_rle_encode_u16(tc_ctx *ctx, const uint16_t *vals, uint64_t N, uint32_t *counts,
                      uint16_t *run_vals, uint64_t *nruns);
/* bytestringBWTFromRLEB (RLE.hs:237-241) = seqFromRLE (RLE/Internal.hs:155-189):
 * (count, Nothing) => one Nothing whatever the count.  N: in capacity, out length. */
int tc_rle_decode(tc_ctx *ctx, const uint32_t *counts, const int16_t *syms, uint64_t nruns,
                  int16_t *sym_out, uint64_t *N);
int tc_rle_decode_u16(tc_ctx *ctx, const uint32_t *counts, const uint16_t *run_vals,
                      uint64_t nruns, uint16_t *vals_out, uint64_t *N);

/* ---- fused pipeline (benchmark path) ------------------------------------- */
/* bytestringToBWT -> bytestringBWTToMTFB -> RLE of the index stream, one call. */
int tc_encode(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_block *out);
/* d_text and out->run_count / out->run_value are device pointers. */
int tc_encode_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_block *out);
/* Inverse chain: RLE -> MTF -> BWT decode; text receives blk->n bytes.
 * The block may come from anywhere: the answer is the reference's on the same runs and list
 * (np.repeat, seqFromMTF over sort(unique(final_list)), magicInverseBWT) -- its text, or
 * TC_ERR_MALFORMED where it throws or its text is not blk->n bytes long (runs that do not
 * expand to n + 1 indices; an index >= the number of distinct list entries in a run of
 * length >= 1; no Nothing, or a second one on the walk).  A run of length 0 indexes nothing,
 * whatever its value.  blk->primary is a hint: a wrong one costs time, not correctness.
 * final_list may be permuted, hold duplicates and hold symbols that never occur.
 * TC_ERR_ARG: sigma > TC_MAX_SIGMA, or a list entry outside -1..255.  sigma == 0 with
 * n > 0 decodes to the empty sequence (MTF/Internal.hs:202-209): TC_ERR_MALFORMED.
 * Nothing behind text[n - 1] is written, whatever the block holds. */
int tc_decode(tc_ctx *ctx, const tc_block *blk, uint8_t *text);
int tc_decode_dev(tc_ctx *ctx, const tc_block *blk, uint8_t *d_text);

/* ---- encoded-block wire format (used by the multi-GPU gather) ----- */
/* The reference has no on-disk / wire format.  Packed form of a tc_block's runs, chosen by sigma
 * (values must be < sigma):
 *   sigma <= 6  (an ACGTN record: 5 letters + sentinel) -- nibble stream: code 0..11 starts a run
 *       (value = code % 6, count = 1 + code / 6); a following 12 / 13 raises a count of 2 to 3 / 4;
 *       a following 14 means "count = next uint32 of the escape list" (counts 0 and >= 5, in run
 *       order); 15 is padding (the stream is dense; its end is padded to a 16-byte boundary).  The
 *       escape list (4 bytes each) follows the nibble body.  `packed` must be 16-byte aligned.
 *   sigma <= 16 -- byte k (k < nruns) = value | (min(count, 15) << 4)
 *   sigma > 16  -- two bytes per run: value low byte, then count (escape 127) | ninth value bit << 7
 *       in both byte forms count >= 15 (127) additionally appends the pair (run index, count) as two
 *       uint32 words to the escape list that follows the bytes at the next 8-byte boundary.
 * *packed_bytes: in = capacity of `packed`, out = bytes used (TC_ERR_CAPACITY: bytes needed);
 * tc_block_packed_bound(nruns, sigma) is always enough.  *nesc returns the number of escapes.
 * All pointers are DEVICE pointers. */
uint64_t tc_block_packed_bound(uint64_t nruns, uint32_t sigma);
int tc_block_pack_dev(tc_ctx *ctx, const tc_block *blk, uint8_t *d_packed, uint64_t *packed_bytes,
                      uint64_t *nesc);
/* Inverse: fills blk->run_count / blk->run_value (device, capacity blk->nruns >= nruns) from
 * packed_bytes bytes; a body that does not hold exactly nruns runs and nesc escapes is
 * TC_ERR_MALFORMED. */
int tc_block_unpack_dev(tc_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, uint64_t nruns,
                        uint32_t sigma, uint64_t nesc, tc_block *blk);

/* ---- encoded-block container ------------------------------------------- */
/* One self-describing byte string per record: a TC_CONTAINER_HEADER-byte little-endian header
 * (magic "TCBLK01", n, primary, nruns, escapes, payload bytes, 64-bit payload checksum, sigma,
 * run format id, final MTF list) followed by the packed runs of tc_block_pack_dev.  The reference
 * has no on-disk / wire format; this is what a caller stores or ships.  Buffers must be 16-byte
 * aligned.  *bytes: in = capacity, out = bytes used (TC_ERR_CAPACITY: bytes needed, as far as known;
 * tc_container_bound is always enough).  Reading verifies magic, sizes and the checksum
 * (TC_ERR_MALFORMED). */
#define TC_CONTAINER_HEADER 640
/* ---- entropy-coded container bodies (an addition to the reference's surface, as the container is) ----
 * What a context's container WRITERS (tc_block_to_container_dev, tc_encode_container_dev, tc_encode_container,
 * tc_encode_stream) put behind the header: TC_CODING_PACKED, the fixed-width packings above (run format id 0..2 =
 * nibble stream / one byte / two bytes per run; the default, and the bytes of every earlier version), or
 * TC_CODING_HUFFMAN, run format id 3, described below.  The setting is state of the context like
 * tc_ctx_set_profile: it survives calls and failed calls; contexts hold it independently; a fresh context is
 * TC_CODING_PACKED.  READERS never look at it: they go by the header's format id, so a stream may mix codings
 * record by record.  Never larger: with TC_CODING_HUFFMAN a record whose Huffman body would not be STRICTLY
 * smaller than its packed body is written packed (format id 0..2), and so is a block with a run of count 0 or a
 * value >= sigma (no token for it) -- tc_container_bound / tc_stream_bound stay sufficient, and the header always
 * says what the body is.  tc_container_coding: coding of a container in HOST memory from its header alone
 * (TC_ERR_MALFORMED if it is none).
 *
 * Body of a format-3 container (all integers little-endian; every part zero-padded to a multiple of 16 bytes):
 *   head       4 x uint32: K (runs per chunk, a power of two; this library writes 1024), nchunks = ceil(nruns / K),
 *              nsyms = sigma + 2, L_max (longest code length; 1 <= L_max <= 12; this library writes 12)
 *   lengths    uint8 length[nsyms]: code length of every token, 0 = the token does not occur and has no code;
 *              every length <= L_max and sum over the coded tokens of 2^-length <= 1
 *   directory  uint32 chunk_bits[nchunks]: number of payload bits of every chunk
 *   payload    uint32 words; chunk k starts at word sum over j < k of ceil(chunk_bits[j] / 32) and occupies
 *              ceil(chunk_bits[k] / 32) words; the payload is exactly the sum of these over all chunks, in words,
 *              padded to 16 bytes
 * Tokens: a run (value v < sigma, count c >= 1) is the token v followed, when c > 1, by the digits of c - 1 in
 *   bijective base 2, least significant first, as tokens RUNA = sigma (digit 1) and RUNB = sigma + 1 (digit 2) --
 *   equivalently: the floor(log2 c) low bits of c, lowest first, RUNA for a 0 bit and RUNB for a 1 bit.  At most 31
 *   digits (c <= 2^32 - 1).  Count 0 has no tokens.
 * Code: canonical.  Coded tokens sorted by (length, token) receive consecutive code values starting from 0, the
 *   value being doubled (shifted left by one) for every step up in length -- code(first) = 0, code(next) =
 *   (code(previous) + 1) << (length(next) - length(previous)).  Only the lengths are stored; a reader depends on
 *   nothing about how they were chosen.  A record with a single distinct token stores length 1 for it.
 * Bits: a code is emitted most significant bit first; bit b of a chunk (b = 0 first) is bit 31 - (b mod 32) of
 *   the chunk's word b / 32.  Chunk k holds the tokens of runs k * K .. min(nruns, (k + 1) * K) - 1 and nothing else:
 *   its first token is a value token, it decodes without looking at any other chunk, and the bits behind
 *   chunk_bits[k] up to the word boundary are zero padding that a reader ignores.  (The directory stores bits, not
 *   words, because zero padding could otherwise be read as digit tokens of the chunk's last run.)  No two chunks
 *   share a word, so a writer needs no read-modify-write across workgroups.
 * Header fields: format = 3, nesc = 0; nruns, body_bytes and the checksum (over the whole body, verified before
 *   anything is decoded) as for the other formats.  The magic stays "TCBLK01": a build without this format
 *   refuses format 3 as inconsistent.  A reader answers TC_ERR_MALFORMED to: K not a power of two, nchunks or
 *   nsyms that do not follow from the header, L_max outside 1..12, a length above L_max, a Kraft sum above 1, a
 *   directory that does not sum to the payload's size, bits that match no code, a chunk that ends inside a code, a
 *   digit before the chunk's first value, more than 31 digits, more or fewer runs in a chunk than it must hold. */
#define TC_CODING_PACKED 0
#define TC_CODING_HUFFMAN 1
int tc_ctx_set_container_coding(tc_ctx *ctx, int coding);   /* TC_ERR_ARG for anything else */
int tc_ctx_get_container_coding(const tc_ctx *ctx);
int tc_container_coding(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, int *coding);
uint64_t tc_container_bound(uint64_t nruns, uint32_t sigma);
int tc_block_to_container_dev(tc_ctx *ctx, const tc_block *blk /* device runs */, uint8_t *d_out, uint64_t *bytes);
/* Text -> container in one call, everything on the device: the bytes of tc_encode_dev followed by
 * tc_block_to_container_dev, without the run arrays in between -- for sigma <= 6 (an ACGTN record) the RLE
 * stage writes the container's nibble stream itself and the container is sealed (escape list, checksum,
 * header) by device kernels.  This is what one step of the multi-GPU path produces and ships
 * (tc_comm_gather).  d_text, d_out: device pointers; d_out 16-byte aligned; *bytes as above
 * (tc_container_bound(n + 2, TC_MAX_SIGMA) is always enough; an ACGTN record needs ~0.45 n). */
int tc_encode_container_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint8_t *d_out, uint64_t *bytes);
/* blk->run_count / run_value: device arrays of capacity blk->nruns (TC_ERR_CAPACITY: blk->nruns = needed). */
int tc_container_to_block_dev(tc_ctx *ctx, const uint8_t *d_in, uint64_t bytes, tc_block *blk);
/* Host side: text -> container and back in one call each; only the compact form crosses PCIe.
 * tc_container_info reads n and nruns from a container in HOST memory. */
int tc_encode_container(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t *bytes);
int tc_container_info(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, uint64_t *n, uint64_t *nruns);
int tc_decode_container(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, uint8_t *text, uint64_t *n_out);

/* ---- chunked stream (texts longer than one record / than HBM) ------------- */
/* A text of any length is cut into records of block_bytes (0 = TC_STREAM_BLOCK_DEFAULT; at most
 * TC_MAX_N; the last record is the remainder; an empty text is one empty record); every record is
 * encoded on its own -- the BWT is global within a record only, as with bzip2's blocks -- and the
 * stream is the records' containers back to back.  Host buffers; record k+1 is copied in and
 * container k-1 copied out while the device encodes record k.  *bytes: in = capacity of `out`,
 * out = bytes used (TC_ERR_CAPACITY: *bytes = tc_stream_bound, always enough).  A stream of one
 * record is byte-identical to tc_encode_container's output. */
#define TC_STREAM_BLOCK_DEFAULT ((uint64_t)1 << 30)
uint64_t tc_stream_bound(uint64_t n, uint64_t block_bytes);
int tc_encode_stream(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t block_bytes, uint8_t *out,
                     uint64_t *bytes);
/* total text length and number of records of a stream in HOST memory (headers only) */
int tc_stream_info(tc_ctx *ctx, const uint8_t *stream, uint64_t bytes, uint64_t *n_total, uint64_t *nblocks);
/* *n_out: in = capacity of `text`, out = bytes written (TC_ERR_CAPACITY: bytes needed); every
 * container's checksum is verified (TC_ERR_MALFORMED). */
int tc_decode_stream(tc_ctx *ctx, const uint8_t *stream, uint64_t bytes, uint8_t *text, uint64_t *n_out);

/* ---- Data.FMIndex -------------------------------------------------------- */
/* bytestringToBWTToFMIndexB (FMIndex.hs:108-111,162-183): C[c] (seqToCc,
 * FMIndex/Internal.hs:275-316), Occ (seqToOccCK :195-259, kept as rank
 * bit-vectors instead of the full sigma x N table) and the suffix array. */
int tc_fm_build(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_fm **out);
/* The same index from a text that already lies in HBM (device pointer; read where it is, never copied or modified;
 * it may be released once the call has returned). */
int tc_fm_build_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_fm **out);
void tc_fm_free(tc_fm *fm);
/* The same index with a SAMPLED suffix array (an addition to the reference's surface).  The suffix array is 4 of the 5 bytes
 * per text byte that locate costs; a sampled index keeps SA[j] only for the rows whose suffix starts at a multiple of sa_rate
 * (text positions 0, sa_rate, 2 sa_rate, ... <= n) and finds the others by walking the LF mapping to the next sampled row.
 * sa_rate: a power of two, 1 .. TC_FM_MAX_SA_RATE; 1 = the full suffix array, the index tc_fm_build makes.  Anything else:
 * TC_ERR_ARG (*out = NULL).  count is unaffected; locate answers the same hits in the same order, at up to sa_rate - 1
 * (on average (sa_rate - 1) / 2) LF steps per hit.
 * Layout of the locate part, instead of the N x 4 bytes of the suffix array:
 *   marks    one more rank bit-vector in the format of the others (64-byte lines {u64 ones-before, 7 x u64 bits}, 448 rows
 *            per line, N / 448 + 1 lines): bit j set iff SA[j] % sa_rate == 0.  One line answers both "is row j sampled"
 *            and "which sample is it".  The row of the whole text (SA = 0, whose last-column symbol is Nothing) is always
 *            marked, so a walk never steps from it.
 *   samples  uint32 samples[n / sa_rate + 1] in ROW order: samples[rank_marks(j)] = SA[j].
 * i.e. 1 + 1/7 + 4 / sa_rate bytes per text byte instead of 5 (tc_fm_device_bytes).  What the saving is NOT: the build
 * still sorts all suffixes, and during the call the full suffix array lies in the ctx's workspace (carved there instead of
 * being allocated for the index), so the peak device memory of a build is what it is for tc_fm_build; the workspace stays
 * with the ctx afterwards as after any call.  The saving is in what the index KEEPS, and in what an export ships. */
#define TC_FM_MAX_SA_RATE 4096
int tc_fm_build_sampled(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sa_rate, tc_fm **out);
int tc_fm_build_sampled_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t sa_rate, tc_fm **out);
/* sa_rate of an index (1: full suffix array; 0: no locate part -- a count-only import, the empty index, NULL) */
uint32_t tc_fm_sa_rate(const tc_fm *fm);
/* device bytes the index holds: part 0 = everything, part 1 = the locate part alone (L + SA, or L + marks + samples),
 * part 2 = the extract part alone (the text samples of tc_fm_build_self: 4 * (n / text_rate + 1); 0 without them; part 0
 * includes it), part 3 = the LCP part alone (tc_fm_build_lcp: 4 * (N + the words of the min tree); 0 without it; part 0
 * includes it); the sizes asked of the allocator, without its rounding.  0 for the empty index or any other part. */
uint64_t tc_fm_device_bytes(const tc_fm *fm, int part);
/* The same index with TEXT SAMPLES as well, so that it can answer what stands at a text position (extract) and the text
 * need not be kept beside it (an addition to the reference's surface).  Beside its locate part (sa_rate as in
 * tc_fm_build_sampled; 1 = the full suffix array) the index keeps, for every text_rate-th text position, the ROW of the
 * suffix that starts there:
 *   isa      uint32 isa[n / text_rate + 1]: isa[k] = the row j with SA[j] = k * text_rate -- 4 / text_rate bytes per text
 *            byte.  The empty suffix (position n) needs no sample: it is row 0 in every index this library builds.
 * text_rate: a power of two, 1 .. TC_FM_MAX_SA_RATE, independent of sa_rate.  Anything else in either rate: TC_ERR_ARG
 * (*out = NULL).  n = 0 gives the empty index (tc_fm_text_rate 0).  count and locate are those of the index
 * tc_fm_build_sampled(sa_rate) makes. */
int tc_fm_build_self(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out);
int tc_fm_build_self_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out);
/* text_rate of an index (0: no text samples -- any other build call, an import without them, the empty index, NULL) */
uint32_t tc_fm_text_rate(const tc_fm *fm);
/* bytestringFMIndexCountS / ...CountP (FMIndex.hs:362-379,411-432) =
 * countFMIndex (FMIndex/Internal.hs:347-438) mapped over the patterns in ONE
 * batched launch; pattern j = pats[offs[j] .. offs[j+1]).  out[j] = count, 0 for
 * Nothing (Q10); result order = pattern order. */
int tc_fm_count(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs,
                uint64_t npat, int64_t *out);
int tc_fm_count_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs,
                    uint64_t npat, int64_t *d_out);
/* bytestringFMIndexLocateS / ...LocateP (FMIndex.hs:475-497,538-563) =
 * locateFMIndex (FMIndex/Internal.hs:448-542): 1-based text positions in SA
 * order.  hit_offs[npat+1] (out) delimits each pattern's hits inside hits[];
 * *nhits: in capacity, out total hits (TC_ERR_CAPACITY sets the needed total). */
int tc_fm_locate(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs,
                 uint64_t npat, uint64_t *hit_offs, uint64_t *hits, uint64_t *nhits);
/* tc_fm_locate with everything in HBM: d_pats, d_offs as tc_fm_count_dev; d_hit_offs [npat + 1] and d_hits [*nhits] are
 * device arrays; *nhits (host): in = capacity, out = total (TC_ERR_CAPACITY sets the needed total and writes nothing to
 * d_hits).  tc_fm_locate is this call between a copy in and a copy out.
 * Locate on a sampled index that was IMPORTED walks caller data: the walk is bounded on any bytes (at most sa_rate - 1
 * steps, every row < N, every sample index within the samples, every position within the text), and a walk that runs into
 * one of its bounds makes the call answer TC_ERR_MALFORMED; on an index this library built it never does. */
int tc_fm_locate_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs,
                     uint64_t npat, uint64_t *d_hit_offs, uint64_t *d_hits, uint64_t *nhits);
/* extract: the text ranges [starts[q], starts[q] + lens[q]) of nq queries, read back from the index.  starts are 1-BASED,
 * exactly as tc_fm_locate answers positions -- tc_fm_extract(hit, |pattern|) returns the pattern -- and every query must lie
 * in the text: 1 <= start and start - 1 + len <= n (len = 0 is allowed for start = 1 .. n + 1); ranges are not clamped.
 * out_offs[nq + 1] (out) delimits each query's bytes inside out[]; *nbytes: in = capacity of out, out = total bytes.
 * A capacity that is too small: TC_ERR_CAPACITY, *nbytes = the needed total, nothing written to out.  A bad query:
 * TC_ERR_ARG, nothing written to out.  An index without text samples (tc_fm_text_rate 0; a count-only import is one):
 * TC_ERR_ARG.  nq = 0: TC_OK.
 * The unit of work is a (query, text_rate-aligned segment) pair: one lane walks the LF mapping from the sampled position at
 * or behind the segment's end down to its start, at most text_rate steps of two dependent random reads each (the
 * last-column byte, then one rank line), so a long range spreads over many lanes and the whole text is n / text_rate + 1
 * independent walks.  Scratch comes from the calling ctx: any number of ctxs may extract from one tc_fm at once.
 * On an IMPORTED index the walk reads caller data: it is bounded on any bytes (the step count is fixed by the query, every
 * row < N, every sample index within the samples, no step from the primary row or from a byte the text does not hold), and
 * a walk that runs into one of its bounds makes the call answer TC_ERR_MALFORMED (its bytes are zeros); on an index this
 * library built it never does. */
int tc_fm_extract(tc_ctx *ctx, const tc_fm *fm, const uint64_t *starts, const uint64_t *lens, uint64_t nq,
                  uint64_t *out_offs, uint8_t *out, uint64_t *nbytes);
/* tc_fm_extract with everything in HBM: d_starts, d_lens [nq], d_out_offs [nq + 1] and d_out [*nbytes] are device arrays;
 * nbytes is a host word.  tc_fm_extract is this call between a copy in and a copy out. */
int tc_fm_extract_dev(tc_ctx *ctx, const tc_fm *fm, const uint64_t *d_starts, const uint64_t *d_lens, uint64_t nq,
                      uint64_t *d_out_offs, uint8_t *d_out, uint64_t *nbytes);
/* Search with mismatches: count and locate within Hamming distance k (an addition to the reference's surface, as the
 * sampled locate and extract are).  Patterns as in tc_fm_count: pattern j = pats[offs[j] .. offs[j+1]), result order =
 * pattern order.
 * COUNT.  For pattern p of length m, out[j] is the number of text positions i, 0 <= i <= n - m, with
 * Hamming(T[i .. i+m), p) <= k.  Substitutions only: there are no insertions or deletions.  A match never runs over the
 * end of the text.  m = 0 gives 0, as tc_fm_count answers Nothing.  m > n gives 0.  m <= k gives n - m + 1.
 * BYTES THAT DO NOT OCCUR IN THE TEXT.  A pattern byte that does not occur in the text can only be a mismatch.  This is a
 * deliberate departure from tc_fm_count: that call stops its loop at such a byte, as the reference does (quirk Q10), and
 * answers for the suffix of the pattern read so far.  Consequence: tc_fm_count_mm(k = 0) equals tc_fm_count for every
 * non-empty pattern all of whose bytes occur in the text, and is 0 where a byte does not.
 * LOCATE.  Positions are 1-based, as in tc_fm_locate.  hit_mm[h] is the Hamming distance of hit h; hit_mm may be NULL.
 * hit_offs[npat + 1], *nhits (in = capacity, out = total) and TC_ERR_CAPACITY (the needed total is set, nothing is written
 * to hits or hit_mm) behave exactly as in tc_fm_locate.  Every position appears once: distinct variant strings have
 * disjoint suffix-array intervals, and the enumeration visits each variant once.  The order inside one pattern's hits is
 * the kernel's enumeration order: it is deterministic, and identical across the host and _dev entry points and across a
 * full and a sampled index of the same text; it is not otherwise specified (in particular it is neither position order
 * nor distance order).
 * ERRORS AND EDGES.  k > TC_FM_MAX_MISMATCH: TC_ERR_ARG.  A null index or null buffers: TC_ERR_ARG.  npat = 0: TC_OK.  The
 * empty index answers zeros.  An index imported without its locate part answers tc_fm_count_mm, and TC_ERR_ARG for
 * tc_fm_locate_mm, as with the exact calls.
 * The _dev forms take everything in HBM (d_hit_offs [npat + 1], d_hits [*nhits], d_hit_mm [*nhits] or NULL; nhits is a host
 * word); the host forms are those calls between a copy in and a copy out.  Scratch comes from the calling ctx: any number
 * of ctxs may search one tc_fm at once.
 * Cost: a bounded depth-first enumeration of the strings within distance k of the pattern that occur in the text, one lane
 * per pattern, one dependent random 64-byte line per node visited; a node with budget left offers every byte value of the
 * text as a substitute, so a search costs about (live nodes with budget left) x sigma lines and grows steeply with k and
 * with the alphabet.  locate runs the enumeration twice (sizes, then hits).  On an IMPORTED index the
 * search reads caller data: it is bounded on any bytes (intervals that leave [1, N] count as empty), and the walk of a
 * sampled index answers TC_ERR_MALFORMED as in tc_fm_locate_dev. */
#define TC_FM_MAX_MISMATCH 3
int tc_fm_count_mm(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t k,
                   int64_t *out);
int tc_fm_count_mm_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t k,
                       int64_t *d_out);
int tc_fm_locate_mm(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t k,
                    uint64_t *hit_offs, uint64_t *hits, uint8_t *hit_mm, uint64_t *nhits);
int tc_fm_locate_mm_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t k,
                        uint64_t *d_hit_offs, uint64_t *d_hits, uint8_t *d_hit_mm, uint64_t *nhits);
/* Factorize: the greedy longest-match parse of patterns against the indexed text, and its inverse (an addition to the
 * reference's surface, as the sampled locate, extract and the search with mismatches are).  Where tc_fm_count answers 0 for
 * a pattern that occurs only in pieces, this call names the pieces: it is the seed step of seed-and-extend, and relative
 * Lempel-Ziv compression of the patterns against the text.  Patterns as in tc_fm_count: pattern j = pats[offs[j] ..
 * offs[j+1]), result order = pattern order.
 * THE PARSE runs right to left, the direction backward search extends a match, and is greedy.  For a pattern p of length m
 * start with j = m and repeat while j > 0: let l be the largest value such that p[j-l .. j) occurs in the text (inside it,
 * never over its end).  l >= 1: the MATCH factor (pos, len = l), pos the 1-based text position, as tc_fm_locate answers
 * them, of the occurrence in the first suffix-array row of the phrase's interval -- the occurrence whose text suffix is
 * lexicographically smallest, the end of the text sorting first; j -= l.  l = 0 (the byte p[j-1] does not occur in the
 * text): the LITERAL factor (pos = that byte's value, len = 0); j -= 1.  len = 0 is never a match, so it marks literals.
 * The factors of one pattern are stored in pattern order, left to right: concatenated they give the pattern back.  The
 * empty pattern has 0 factors.  The answer is fully determined: the same through the host and _dev entries and on a full
 * and a sampled index of one text.
 * fac_offs[npat + 1] (out) delimits each pattern's factors inside fac_pos[] / fac_len[]; *nfac: in = capacity of both, out =
 * total factors.  A capacity that is too small: TC_ERR_CAPACITY, *nfac = the needed total, nothing written to fac_pos or
 * fac_len.  fac_pos = fac_len = NULL with capacity 0 is the sizes-only form: TC_OK, fac_offs and the total written -- the
 * factor count of every pattern, a similarity measure on its own.
 * UNFACTORIZE expands factor lists back to bytes from an index that holds text samples (tc_fm_text_rate > 0): a match is the
 * text range [pos, pos + len), a literal its byte; unfactorize(factorize(p)) = p for every byte string p, and the text
 * itself need not be kept.  out_offs[npat + 1], out and *nbytes as in tc_fm_extract (TC_ERR_CAPACITY: the needed total,
 * nothing written to out).  A bad list -- fac_offs[0] != 0, fac_offs decreasing, a match with pos = 0 or pos - 1 + len > n,
 * a literal with pos > 255 -- is TC_ERR_ARG with nothing written to out.
 * ERRORS AND EDGES.  A null index or null buffers: TC_ERR_ARG.  npat = 0: TC_OK.  The empty index: every byte is a literal.
 * Factorize on an index imported without its locate part: TC_ERR_ARG.  Unfactorize without text samples: TC_ERR_ARG.
 * The _dev forms take everything in HBM (nfac / nbytes are host words); the host forms are those calls between a copy in and
 * a copy out.  Scratch comes from the calling ctx: any number of ctxs may use one tc_fm at once.
 * Cost: one lane per pattern, one dependent random 64-byte line per pattern symbol (per two symbols with pair vectors) plus
 * about one per factor; the parse runs twice (sizes, then factors), and on a sampled index one locate walk per match factor
 * follows.  Unfactorize is one flat extract over all factors.  On an IMPORTED index the parse reads caller data: it is
 * bounded on any bytes (intervals that leave [1, N] count as empty, every turn consumes a byte or closes a phrase), and the
 * walks answer TC_ERR_MALFORMED as in tc_fm_locate_dev and tc_fm_extract_dev. */
int tc_fm_factorize(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat,
                    uint64_t *fac_offs, uint64_t *fac_pos, uint32_t *fac_len, uint64_t *nfac);
int tc_fm_factorize_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat,
                        uint64_t *d_fac_offs, uint64_t *d_fac_pos, uint32_t *d_fac_len, uint64_t *nfac);
int tc_fm_unfactorize(tc_ctx *ctx, const tc_fm *fm, const uint64_t *fac_offs, const uint64_t *fac_pos, const uint32_t *fac_len,
                      uint64_t npat, uint64_t *out_offs, uint8_t *out, uint64_t *nbytes);
int tc_fm_unfactorize_dev(tc_ctx *ctx, const tc_fm *fm, const uint64_t *d_fac_offs, const uint64_t *d_fac_pos,
                          const uint32_t *d_fac_len, uint64_t npat, uint64_t *d_out_offs, uint8_t *d_out, uint64_t *nbytes);
/* Matching statistics and maximal exact matches (an addition to the reference's surface, as factorize is).  Where
 * tc_fm_count asks whether the whole pattern occurs and tc_fm_factorize for one greedy parse, this asks, for EVERY position
 * of a pattern, how long a match starts there and where it occurs: what an aligner, a read classifier or a similarity
 * search seeds from.  Patterns as in tc_fm_count: pattern j = pats[offs[j] .. offs[j+1]).
 * THE INDEX needs an LCP part: tc_fm_build_lcp is tc_fm_build_self plus
 *   lcp      uint32 lcp[N]: exactly the array tc_lcp_array_dev defines (lcp[0] = 0) -- 4 bytes per text byte, which doubles
 *            the locate part of a full index
 *   lmin     a min tree over it with fan-out 64: level 1 entry b = min lcp[64 b .. 64 b + 64), level k + 1 over level k
 *            the same way, up to the first level of at most 64 entries; every level rounded up to a multiple of 4 words,
 *            less than N / 63 + 4 per level words in all
 * sa_rate as in tc_fm_build_sampled; text_rate 0 (no text samples) or as in tc_fm_build_self; anything else: TC_ERR_ARG
 * (*out = NULL).  n = 0 gives the empty index.  tc_fm_has_lcp: 1 / 0.  The LCP part is NOT exported: tc_fm_export_dev of
 * such an index ships, byte for byte, what it ships for the same index built without the part, and an import never has
 * one.  Every other call answers on such an index what it answers without the part.
 * MATCHING STATISTICS.  For a pattern p of length m and every 0 <= i < m, at index offs[j] + i of the result arrays:
 *   ms_len   the largest l such that p[i .. i+l) occurs in the text (inside it, never over its end); l = 0 means that the
 *            byte p[i] does not occur in the text
 *   ms_pos   the 1-based text position, as tc_fm_locate answers them, of that string's occurrence in the FIRST
 *            suffix-array row of its interval -- the convention of tc_fm_factorize; 0 where l = 0
 *   ms_occ   the number of text occurrences of p[i .. i+l), the interval's width; 0 where l = 0
 * ms_pos and ms_occ may each be NULL; ms_len must not.  The answer is fully determined: the same through the host and _dev
 * entries, and on a full and a sampled index of one text, with or without text samples.
 * MAXIMAL EXACT MATCHES of pattern p with min_len >= 1 are the triples (i, ms_pos[i], ms_len[i]) with ms_len[i] >= min_len
 * and (i = 0 or ms_len[i-1] <= ms_len[i]).  ms_len[i-1] <= ms_len[i] + 1 always holds, so the second condition says exactly
 * that the match cannot be extended to the left; by the definition of ms_len it cannot be extended to the right either.
 * These are the matches not contained in a longer match of the same pattern.  The MEMs of one pattern are stored in
 * increasing i: mem_start = i (0-based in the pattern), mem_pos, mem_len.  mem_offs[npat + 1] (out) delimits each pattern's
 * MEMs; *nmem: in = capacity of the three arrays, out = total.  A capacity that is too small: TC_ERR_CAPACITY, *nmem = the
 * needed total, nothing written to the three arrays.  mem_start = mem_pos = mem_len = NULL with capacity 0 is the sizes-only
 * form: TC_OK, mem_offs and the total written.  All occurrences of a MEM: tc_fm_locate on the substring.
 * ERRORS AND EDGES.  A null index or null buffers: TC_ERR_ARG.  A non-empty index without the LCP part (tc_fm_has_lcp 0:
 * every other build call, every import): TC_ERR_ARG.  min_len = 0: TC_ERR_ARG.  npat = 0: TC_OK.  The empty index answers
 * all zeros and no MEMs.  The _dev forms take everything in HBM (nmem is a host word); the host forms are those calls
 * between a copy in and a copy out.  Scratch comes from the calling ctx: any number of ctxs may query one tc_fm at once.
 * Cost: one lane per pattern, one dependent random 64-byte line per pattern symbol (single-symbol steps: a two-symbol step
 * does not yield the interval of the position between), one 4-byte store per symbol and array, and where a step fails a
 * shrink to the parent interval: two LCP reads and two searches in the min tree of at most 2 * 64 words per level each,
 * whatever the text.  On a sampled index one locate walk per position follows when ms_pos is asked for
 * (tc_fm_mems: per MEM). */
int tc_fm_build_lcp(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out);
int tc_fm_build_lcp_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out);
int tc_fm_has_lcp(const tc_fm *fm);
int tc_fm_match_stats(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat,
                      uint32_t *ms_len, uint64_t *ms_pos, uint32_t *ms_occ);
int tc_fm_match_stats_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat,
                          uint32_t *d_ms_len, uint64_t *d_ms_pos, uint32_t *d_ms_occ);
int tc_fm_mems(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t min_len,
               uint64_t *mem_offs, uint64_t *mem_start, uint64_t *mem_pos, uint32_t *mem_len, uint64_t *nmem);
int tc_fm_mems_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat,
                   uint32_t min_len, uint64_t *d_mem_offs, uint64_t *d_mem_start, uint64_t *d_mem_pos, uint32_t *d_mem_len,
                   uint64_t *nmem);
/* seqToCc / seqFromFMIndex views for the Haskell shim: present symbols (sorted,
 * Nothing first) with C[c]; and L / primary. */
int tc_fm_info(const tc_fm *fm, uint64_t *N, uint32_t *sigma, int16_t *c_sym, uint64_t *c_val,
               uint64_t *primary);

/* Replication of a built index over the GPUs of a node (FM-count shards by pattern batch,
 * the index is broadcast once): the index as ONE device byte string (header, C / code tables, rank
 * bit-vectors; with_locate != 0 adds the last column and the suffix array that tc_fm_locate needs -- of a sampled index
 * the last column, the marks and the samples, and the header's formerly reserved word carries sa_rate; a full index
 * writes 0 there, its export is byte for byte what it was; an index with text samples (tc_fm_build_self) ships them
 * behind the locate part, 256-byte aligned like every part, and its header's with_locate word is 1 | text_rate << 8, while
 * an index without them writes 1 as ever; with_locate == 0 ships neither -- ) and
 * back.  The caller moves the bytes (RCCL broadcast); tc_fm_import_dev checks the header
 * (TC_ERR_MALFORMED; for a sampled index also: the rate, the sizes that follow from N and the rate, and that the marks hold
 * exactly one bit per sample; for text samples: the rate, the size that follows from n and the rate, that position 0 is
 * sampled at the primary row and that every sample is a row) and copies out of d_in, which may be released afterwards.  An index imported
 * without the locate part answers tc_fm_count only (tc_fm_locate: TC_ERR_ARG).  Buffers 16-byte
 * aligned.  *bytes: in = capacity, out = bytes used (TC_ERR_CAPACITY: bytes needed).  The byte string is BUILD-SPECIFIC
 * (it carries a format version: "TCFMI02" since round 3; an export of another version is refused with a message that
 * says so): it travels between the ranks of one job, it is not an archive format.
 * WHAT AN IMPORTED INDEX MAY HOLD.  The import checks what is listed above and nothing else: the rank vectors, the last
 * column, the samples' values and the suffix array are taken as they come, and the queries meet them as caller data.  The
 * rule for every query entry (count, locate, extract, the _mm forms, factorize, host and _dev alike): a malformed body is
 * answered by TC_ERR_MALFORMED, at the import or at the query, or by TC_OK with the answer the contents define -- the one
 * the written rules of the kernels give on those bytes: a search interval is stepped from, counted or reported only when
 * 1 <= s <= e <= N, anything else counts as no occurrence; a locate on a full index answers the suffix array's word + 1,
 * whatever it is; a walk that runs into one of its bounds is TC_ERR_MALFORMED -- and every kernel stays inside the
 * index's parts: no content makes one read or write outside them, or spin.  tests/fm_wire_ref.py is that definition in
 * numpy; tests/test_gpu_fm_import_foreign.py holds the entries to it. */
uint64_t tc_fm_export_bound(const tc_fm *fm, int with_locate);
int tc_fm_export_dev(tc_ctx *ctx, const tc_fm *fm, int with_locate, uint8_t *d_out, uint64_t *bytes);
int tc_fm_import_dev(tc_ctx *ctx, const uint8_t *d_in, uint64_t bytes, tc_fm **out);

/* ---- the exchange of the multi-GPU path ------------------------------------------ */
/* One process per GPU, one tc_ctx per process, one record per GPU: nothing is exchanged during the
 * encode.  A tc_comm is an RCCL communicator over the ranks of the job, bound at run time (dlopen: a
 * process that never calls tc_comm_* never loads RCCL; failures are TC_ERR_NCCL).  Rank 0 obtains an id
 * with tc_comm_unique_id and hands its TC_COMM_ID_BYTES bytes to the other ranks by whatever channel
 * started them (environment, file, MPI ...); then every rank calls tc_comm_create (collective).
 *
 * tc_comm_gather (collective): the variable-size gather of one container (tc_block_to_container_dev)
 * per rank on `root`.  Sizes travel by an all-gather of one word per rank (sizes[world], host, out on
 * every rank); then the root receives rank r's bytes at d_recv + r * slot_bytes (its own container is
 * copied there too) in ONE group of point-to-point transfers -- it ingests on all of its xGMI links at
 * once.  A size above slot_bytes is TC_ERR_CAPACITY on EVERY rank (before anything is sent).  The call
 * returns once the transfers are POSTED on the communicator's own stream: the gather of record k overlaps
 * the encode of record k + 1; d_container and d_recv belong to the exchange until tc_comm_wait returns.
 * tc_comm_broadcast (collective, complete on return): `bytes` of d_buf from root to all (an exported
 * FM-index, tc_fm_export_dev -> tc_fm_import_dev).  All buffers are device pointers. */
#define TC_COMM_ID_BYTES 128
typedef struct tc_comm tc_comm;
int tc_comm_unique_id(tc_ctx *ctx, uint8_t *id /* [TC_COMM_ID_BYTES] */);
int tc_comm_create(tc_ctx *ctx, const uint8_t *id, int rank, int world, tc_comm **out);
void tc_comm_destroy(tc_comm *comm);
int tc_comm_gather(tc_comm *comm, int root, const uint8_t *d_container, uint64_t bytes, uint8_t *d_recv,
                   uint64_t slot_bytes, uint64_t *sizes);
int tc_comm_wait(tc_comm *comm);
/* The exchange overlaps the next record's encode; to keep RCCL's workgroups from holding back the encode's
 * partition levels (which want whole CUs), the communicator's stream is restricted to TC_COMM_CUS compute units
 * (environment; default 8 when world > 1, one per XCD; 0: unrestricted) and the context's partition levels
 * split their work over the others.  Returns how many CUs this communicator is restricted to (0: none). */
int tc_comm_reserved_cus(const tc_comm *comm);
int tc_comm_broadcast(tc_comm *comm, int root, uint8_t *d_buf, uint64_t bytes);

/* ---- synthetic inputs, generated on the device ------------- */
/* kind 0: iid ACGTN, kind 1: printable ASCII; the classes away from iid text that bench.py reports beside the headline
 * (round 4; every byte a function of (kind, seed, position) alone): 2 genome-like (iid ACGT with a 300-bp repeat family in
 * ~10 % of the sequence, poly-A tracts, (CA)n), 3 Zipf-distributed words of 2 .. 9 letters from a 20 000-word vocabulary,
 * 4 runs (a letter repeats with probability 0.9), 5 a 4096-byte block repeated, 6 an assembly with gaps (iid ACGT, one run of
 * n / 64 'N's and sixteen of n / 4096).  d_out is a device pointer. */
int tc_generate_dev(tc_ctx *ctx, int kind, uint64_t seed, uint64_t n, uint8_t *d_out);

#ifdef __cplusplus
}
#endif
#endif /* TEXTCOMP_H */
