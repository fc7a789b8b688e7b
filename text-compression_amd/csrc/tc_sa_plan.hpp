// tc_sa_plan.hpp -- the decisions of the suffix-sort driver (tc_sa_host.hpp) that need no device: the knobs, which way
// round 0 goes, and when a doubling round becomes a chain round.  Plain C++ without a HIP header, so that
// host/check/sa_chain_policy.cpp can drive it under a host sanitizer.
#pragma once
#include <math.h>
#include <stdint.h>

// Every environment variable the suffix sort reads, with its default.  Constructing one reads them all; sa_run makes
// one at its top: per call, because callers change the environment between calls on one context.  env_int(name, default)
// is the includer's (tc_encode_host.hpp; the host check has its own, which answers the default).
// (TC_SA_MSD_MIN_LOG2 is read where the workspace is carved: msd_min_n.  TC_DBG_TICKET_TRIP and the variables of the
// radix sort itself are read where they are used.)
struct SaKnobs {
    int trace = env_int("TC_SA_TRACE", 0);   // 1 = decisions and wall time per step on stderr (a stream sync each), 2 = also buffer addresses and tied-set checksums
    int fields = env_int("TC_SA_FIELDS", 0);   // > 0 forces the number of key fields P (and keeps round 0 from widening it or going MSD)
    int bin_min_log2 = env_int("TC_SA_BIN_MIN_LOG2", 25);   // dense ranks of sets of at least 2^this members are stored by regions
    int kb_onehist = env_int("TC_KB_ONEHIST", 1);   // 0 = a digit histogram per pass even where one shared histogram would do
    int keygen_fused = env_int("TC_KEYGEN_FUSED", 1);   // 0 = write the round-0 keys before the first pass instead of generating them inside it
    int xcd_group = env_int("TC_XCD_GROUP", 1);   // 0 = round 0's radix passes draw tiles from a single counter
    int finish = env_int("TC_SA_FINISH", 1);   // 0 = no finish pass: round 0 goes the full path
    int dense = env_int("TC_SA_DENSE", 0);   // 1 = dense ranks (and the full path) whatever the size of the tied set
    int global_passes = env_int("TC_SA_GLOBAL_PASSES", 0);   // > 0 forces the number of global passes G of the LSD way
    int sample = env_int("TC_SA_SAMPLE", 1);   // 0 = no collision sample before round 0
    int msd = env_int("TC_SA_MSD", 1);   // 0 never the MSD way, 1 by the selectors, 2 whenever it is possible, 3 also repeat-rich text by the big finish
    int msd_big = env_int("TC_SA_MSD_BIG", 0);   // 1 = the big finish instance whatever the expected bucket
    int msd_max_dups = env_int("TC_SA_MSD_MAX_DUPS", 8);   // sample duplicates (above the iid expectation) the MSD way tolerates
    int keyround = env_int("TC_SA_KEYROUND", 1);   // 0 = no key round for the whole buckets of the big finish
    int msd_keyonly = env_int("TC_SA_MSD_KEYONLY", 1);   // 0 the levels always move suffix starts, 1 keys only when few ties are expected, 2 whenever no array is asked for
    int keygen_hash = env_int("TC_KEYGEN_HASH", 1);   // 0 = byte -> code through the table even where the register hash would do
    int msd_grid = env_int("TC_MSD_GRID", 0);   // > 0 caps the workgroups of the MSD levels
    int msd_joint = env_int("TC_SA_MSD_JOINT", 1);   // 0 = level 3 counts its own digits instead of taking them from level 2
    int msd_split = env_int("TC_MSD_SPLIT", 1);   // 0 = level 1 of the key-only levels writes 64-bit keys instead of two arrays of halves (and the joint count reads all 8 bytes)
    int msd_dir = env_int("TC_MSD_DIR", 1);   // 0 = the aligned level walks the parent tables at every boundary instead of keeping a directory of its live parents in LDS
    int tied_probe = env_int("TC_TIED_PROBE", 1);   // 0 = the tied suffixes of the key-only levels are always found again through the byte image of codes (tied_probe_kernel), never by codes from the register table (tied_probe_w_kernel)
    int msd_finish_lut = env_int("TC_MSD_FINISH_LUT", 1);   // 0 = the finish bins by key bits instead of equal-mass intervals
    int msd_finish_ko = env_int("TC_MSD_FINISH_KO", 1);   // 0 = the generic finish instance for the key-only levels
    int tier2 = env_int("TC_SA_TIER2", 1);   // 0 = no fix pass for over-long buckets of the LSD finish (the full path then)
    int tiny = env_int("TC_SA_TINY", 1);   // 0 = tied sets of one window are ordered and tabled by the general kernels
    int seg = env_int("TC_SA_SEG", 1);   // 0 = doubling rounds by radix passes, never the segmented sort
    int seg_min = env_int("TC_SA_SEG_MIN", 1 << 16);   // members from which a round (and the key round) uses the segmented sort
    int deep = env_int("TC_SA_DEEP", 1);   // 0 = the full path keeps the fields the entropy estimate chose
    int accel_min = env_int("TC_SA_ACCEL_MIN", 1 << 20);   // tied members from which the sparse table gets its bitmap and key directory
    int kdir_search = env_int("TC_SA_KDIR_SEARCH", 0);   // 1 = the key directory by a search per entry instead of mark and fill
    int h_start = env_int("TC_SA_H_START", 0);   // > 0 forces the depth the doubling starts from
    int chain = env_int("TC_SA_CHAIN", 1);   // 0 never a chain round, 1 by ChainPolicy, 2 every round that can
};

// ---- round 0: which way ------------------------------------------------------------------------------------------
// What the decision looks at.  The limits are the kernels' (tc_msd.hpp, tc_sa.hpp), handed in by the caller.
struct Round0In {
    double entropy;        // bits per symbol (sa_choose_config)
    uint32_t w, s, P;      // bits per field, symbols per field, fields chosen for the full path
    uint64_t N;            // suffixes
    bool msd_carved;       // the workspace holds the MSD tables (msd_wanted said so)
    bool want_sa;          // the caller asked for the suffix array itself
    uint32_t sample_dups;  // duplicates among the collision sample (0: not taken)
    int msd_levels;                       // MSD_LEVELS
    uint32_t cap_small, cap_big;          // MSDF_CAP_SMALL, MSDF_CAP_BIG
    uint32_t samp_n, tied_max;            // SAMP_N, TP_MAX_TIED
};
struct Round0Plan {
    int G, topbits;   // global passes of the LSD way, and the key bits they order
    bool msd_cand;    // the MSD way is possible at all (alphabet, length, no forced fields or passes)
    uint32_t P;       // fields of the round-0 key (the finish pass ranks by all remaining bits, so more cost nothing)
    bool try_msd, msd_big, keyonly, keyround;
};

// Global passes: enough top bits that an iid text of this entropy leaves ~4 suffixes per bucket, and few enough
// remaining bits for the finish pass (<= 32).  Reads in.{entropy, w, s, P, N, msd_carved}; leaves G, topbits, msd_cand.
static inline void sa_round0_depth(const Round0In &in, const SaKnobs &K, Round0Plan &pl) {
    const int keybits = (int)(in.P * in.w);
    double e8 = in.w == 8 ? in.entropy * in.s : in.entropy * 8.0 / in.w;
    int G = e8 > 1e-9 ? (int)ceil((log2((double)in.N) - 4.0) / e8) : 64;  // ~16 suffixes per bucket at most
    if (G < (keybits - 32 + 7) / 8) G = (keybits - 32 + 7) / 8;
    if (G < 1) G = 1;
    if (K.global_passes > 0) G = K.global_passes;
    // a candidate for the MSD way sorts by 7 fields: its LSD fallback then needs >= 3 global passes
    pl.msd_cand = in.w == 8 && in.msd_carved && K.fields == 0 && K.global_passes == 0;
    if (pl.msd_cand && G < in.msd_levels) G = in.msd_levels;
    pl.G = G;
    pl.topbits = 8 * G < keybits ? 8 * G : keybits;
    pl.P = in.P;
}

// The rest, once the sample is in (only called when the finish pass can take the remaining bits and the sample is not
// hopeless).  Reads everything of `in` and pl.{topbits, msd_cand}; leaves P, try_msd, msd_big, keyonly, keyround.
//
// Round 0, two ways.  MSD (tc_msd.hpp; long texts over a small alphabet): three partition levels by field 0, 1, 2 with
// whole-line stores, then every level-3 bucket ordered in LDS.  LSD (tc_radix.hpp): the top fields by stable passes,
// then finish_kernel.  The MSD way is for texts that look iid at the depth of its levels: (i) the entropy estimate
// puts a level-3 bucket well under the finish kernel's chunk, (ii) the sample met next to no repeated 12-symbol prefix
// (repeat-rich DNA has dozens among 8192; iid text of this length none) -- otherwise the attempt would be paid for and
// then thrown away.
static inline void sa_round0_plan(const Round0In &in, const SaKnobs &K, Round0Plan &pl) {
    // fields beyond the globally sorted ones cost no pass here (the finish pass ranks by all remaining bits at once),
    // so take as many as fit: fewer suffixes stay tied
    if (K.fields == 0) {
        uint32_t pf = (uint32_t)((pl.topbits + 32) / (int)in.w);
        if (pf > 56 / in.w) pf = 56 / in.w;
        if (pf > pl.P) pl.P = pf;
    }
    const double field_bits = in.entropy * in.s < 8.0 ? in.entropy * in.s : 8.0;
    const double lvl_bits = field_bits * in.msd_levels;
    // expected level-3 bucket: a third of a small chunk (5-letter DNA at 1 GiB) -> the small finish instance; up to
    // ~5/8 of a big chunk (4-letter DNA at 1 GiB: 4096) -> the big one, which also writes the keys in final order
    // (rank lookups by binary search: its buckets are too long to scan)
    const double msd_bucket = (double)in.N / exp2(lvl_bits);
    pl.msd_big = msd_bucket > (double)in.cap_small / 3.0 || K.msd_big != 0;
    const bool msd_fits = msd_bucket <= (double)in.cap_big * 0.8;
    // (what an iid text of this entropy leaves among the samples at the sampled depth, with slack)
    const double iid_dups = (double)in.samp_n * in.samp_n / 2.0 / exp2(field_bits * (pl.topbits / 8));
    const bool msd_iid = (double)in.sample_dups <= (double)K.msd_max_dups + 3.0 * iid_dups;
    // (the big instance copes with repeats -- over-long buckets leave as tied groups, ranks of untied suffixes come by
    // binary search in its sorted keys -- but repeat-rich DNA is slower this way than by the LSD way, whose finish
    // orders 14+ symbols instead of 12: 1 GiB genome-like 188 ms against 116 ms.  So the sample decides for both
    // instances.)
    // (Sending repeat-rich DNA this way as well was tried -- the big instance's whole buckets go through the key round
    // and come out tied on all 21 symbols -- but on such text the levels and the big finish themselves are slow: 8.1
    // instead of 5.9 ms per level and 32 instead of 7 ms for the finish at 1 GiB (one workgroup per level-3 parent: the
    // parents of the repeat family are the tail), 112 ms against 99 by the LSD way.  TC_SA_MSD=3: that experiment; the
    // key round itself stays for the whole buckets an iid-looking text still has.)
    pl.keyround = K.keyround != 0;
    pl.try_msd = pl.msd_cand && pl.P == 7 &&
                 (K.msd == 2 || (msd_fits && (msd_iid || (pl.msd_big && pl.keyround && K.msd == 3))));
    // no suffix array asked for (encode, BWT): the levels can move keys only (tc_msd.hpp, VALS = false).  Both finish
    // instances; the big one's over-long buckets (whole tied groups: msd_whole_kernel works from the suffix starts) send
    // the text through the levels again with the starts moving along -- so it is only tried when few ties are expected:
    // an iid text of this entropy leaves about N^2 / 2^(entropy x key symbols) suffixes equal on the whole key (1 GiB:
    // 5-letter DNA 2 300, measured 2 404; 4-letter DNA 262 000, measured 261 586 -- more than the table of tied keys is
    // made for)
    const double tied_est = (double)in.N * (double)in.N / exp2(in.entropy * (double)(pl.P * in.s));
    pl.keyonly = !in.want_sa && (tied_est < (double)in.tied_max / 4.0 || K.msd_keyonly == 2) && K.msd_keyonly != 0;
}

// ---- doubling: when a round becomes a chain round ----------------------------------------------------------------
// Chain rounds (tc_chain.hpp): when a round sheds next to nothing (periodic text, a long run of one symbol) the next one
// orders every group by how long its members keep seeing the same thing at + h, + 2 h, .. -- two passes of the same sort
// at one h.  TC_SA_CHAIN: 0 never, 1 (default) after a PLAIN round that resolved < 1/256 of a set of >= 2^20 members,
// 2 every round.
// (Not in the very first doubling round, however few suffixes round 0 resolved: a chain is cut wherever two residue
// classes of the period share their h symbols -- members of the merged group see two different ranks at + h, one of them
// is not the reference -- and the cut repeats with the period, so all members of a class get the SAME k.  One such
// coincidence in a 1 MiB period at h = 21 left 97 % of a 1 GiB record tied after the chain round; a plain round first
// splits the merged groups, and 2 h symbols rarely coincide: chain round at 42 -> everything resolved.)
// Back-off: text that is repetitive without being periodic (a Fibonacci or Thue-Morse word: every round keeps nearly all
// of it tied, but its chains are short) would pay a chain round -- two passes -- at every other doubling for nothing
// (2^28 bytes: 762 instead of 538 ms).  A chain round that resolved less than an eighth of its members makes the next
// attempt wait 2, 4 plain rounds; after three such rounds there are no more (forced rounds, TC_SA_CHAIN=2, ignore this).
struct ChainPolicy {
    int mode;             // TC_SA_CHAIN
    int keymode = 0;      // the pass at hand: 0 plain (key2 = rank[i + h]); 1 a chain round's first pass (the chain code);
                          // 2 its second (the rank the member's terminal sees)
    uint64_t prev_mm = 0; // members of the last plain doubling round (0: none yet, or a chain round came since)
    int chain_fail = 0, chain_wait = 0;
    uint64_t chain_m0 = 0;   // members the chain round at hand started with

    explicit ChainPolicy(int mode_) : mode(mode_) {}

    // Does the pass that is about to sort m members at depth h (hh: h capped at N) start a chain round?  Only a
    // segmented round can.  Yes: the pass becomes the round's first (keymode 1).
    bool start(bool seg_round, uint32_t hh, uint64_t h, uint64_t N, uint64_t m) {
        if (keymode != 0 || !seg_round || hh < 4 || h >= N || mode == 0) return false;
        if (mode != 2 && !(m >= (1u << 20) && prev_mm > 0 && (prev_mm - m) * 256 < prev_mm && chain_wait == 0 && chain_fail < 3))
            return false;
        keymode = 1;
        chain_m0 = m;
        return true;
    }
    // Accounts for a finished pass over m members of which m_left stay tied.  True: the next pass doubles h (false:
    // it is the chain round's second pass, at the same h).
    bool finish(uint64_t m, uint64_t m_left) {
        if (keymode == 1) {
            keymode = 2;
            return false;
        }
        if (keymode == 2) {
            if ((chain_m0 - m_left) * 8 < chain_m0) chain_wait = 1 << ++chain_fail;
        } else if (chain_wait > 0) chain_wait--;
        prev_mm = keymode == 2 ? 0 : m;
        keymode = 0;
        return true;
    }
};
