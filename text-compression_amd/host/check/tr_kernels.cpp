// Stand-alone host check of the tandem-repeat kernel (csrc/tc_tr.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/tr_kernels.cpp -o tr_kernels && ./tr_kernels
// TC_FM_MS_HOST_CHECK compiles tr_cand_kernel, the range minimum of csrc/tc_lz.hpp and the upward row search of
// csrc/tc_fm_ms.hpp it calls as plain C++, as host/check/rep_kernels.cpp does for the repeats kernel: the HIP keywords
// defined away, a workgroup of one lane, the lanes of a grid run one after another.  Everything is built naively --
// the suffixes of the text and of its reverse sorted directly, the LCP arrays by comparing neighbours, the inverse arrays
// by scatter, the min trees by fm_lmin_kernel level over level at fan-outs 4 and 64 -- in heap blocks of exactly the
// entries the library's arrays hold, so a read one element outside any of them stops the run.  Every position's two
// candidate words, for several filters, are compared with brute force twice: slot by slot with the rule evaluated by
// scanning the text (the next position with a smaller / larger suffix, then byte comparisons both ways), and as a whole
// with the runs of the definition found by shifting the text against itself -- every run once, no other triple.  Texts:
// unary, periodic (2, 3, 7), periodic with edits, Fibonacci, random over 1, 2, 4 and 256 letters, a text followed by its
// copy, skewed two-letter texts, and texts built so that a search or a range minimum has to go to the top of the tree;
// lengths 1 .. 2200, and 2600 for the last kind.  The program asserts that at fan-out 4 both searches and both range
// minima reached every level of the tree, and reports the levels.  The scatter, count, fill
// and order kernels need atomics or a device scan: they are checked on the device only.
#include <tuple>

#define TC_FM_MS_HOST_CHECK
#include "tc_tr.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

// ---- isa, lcp and the LCP min tree of one text, naively, in blocks of the library's sizes --------------------------------
struct Esa {
    u32 N = 0;
    std::unique_ptr<u32[]> isa, lcp;
};
static void build_esa(Esa &e, const Bytes &text) {
    const std::vector<u32> sa = sort_suffixes(text);
    e.N = (u32)sa.size();
    e.isa = block_of(inverse_of(sa));
    e.lcp = block_of(lcp_of(text, sa));
}

// ---- the runs of the definition: for every period the maximal stretches of text[k] == text[k + p], at least p long,
// whose period p is the smallest (a smaller one would, with p, make their common divisor a period: Fine and Wilf)
typedef std::tuple<u32, u32, u32> Run;     // start, period, length
static std::vector<Run> runs_by_shifting(const Bytes &t) {
    const u32 n = (u32)t.size();
    std::vector<Run> out;
    for (u32 p = 1; 2 * p <= n; p++) {
        for (u32 a = 0; a + p < n;) {
            if (t[a] != t[a + p]) {
                a++;
                continue;
            }
            u32 b = a;
            while (b + p < n && t[b] == t[b + p]) b++;          // pairs [a, b)
            if (b - a >= p) {
                const u32 s = a, len = b - a + p;
                bool smallest = true;
                for (u32 q = 1; q < p && smallest; q++) {
                    if (p % q) continue;
                    bool period = true;
                    for (u32 k = s; k + q < s + len && period; k++) period = t[k] == t[k + q];
                    if (period) smallest = false;
                }
                if (smallest) out.push_back(Run(s, p, len));
            }
            a = b + 1;
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}

static bool passes(const TrFilter &f, u32 p, u32 len) {
    return p >= f.min_period && (f.max_period == 0 || p <= f.max_period) && len / p >= f.min_copies && len >= f.min_len;
}

static u64 g_texts = 0, g_positions = 0, g_runs = 0, g_tie_broken = 0;
static u32 g_top[8] = {};       // [fan-out 4: 0 .. 3, fan-out 64: 4 .. 7] the highest level each of the four climbs reached
static u32 g_nlev[2] = {};      // the deepest tree seen at each fan-out
static void check_text(const Bytes &text, u32 lf) {
    const u32 n = (u32)text.size(), N = n + 1;
    Esa F, R;
    build_esa(F, text);
    build_esa(R, Bytes(text.rbegin(), text.rend()));
    auto comp = block<u32>(N);
    for (u32 j = 0; j < N; j++) comp[j] = N - 1 - F.isa[j];
    const MinTree ti = min_tree_of(F.isa.get(), N, lf), tc = min_tree_of(comp.get(), N, lf), tl = min_tree_of(F.lcp.get(), N, lf),
                  tr = min_tree_of(R.lcp.get(), N, lf);
    auto text_blk = block<u8>(n);
    std::copy(text.begin(), text.end(), text_blk.get());
    auto c_start = block<u32>(2 * (size_t)n);
    auto c_pl = block<u64>(2 * (size_t)n);
    const std::vector<Run> all = runs_by_shifting(text);
    EXPECT(all.size() < std::max(n, 1u));           // the runs theorem
    const TrFilter filters[] = {{1, 0, 2, 1}, {2, 0, 2, 1}, {1, 3, 2, 1}, {1, 0, 3, 1}, {1, 0, 2, 9}, {2, 7, 3, 12}};
    for (const TrFilter &f : filters) {
        for (size_t k = 0; k < 2 * (size_t)n; k++) c_start[k] = 0xffffffffu, c_pl[k] = ~0ull;
        launch(n, [&] {
            tr_cand_kernel(text_blk.get(), n, F.isa.get(), ti.lmin.get(), comp.get(), tc.lmin.get(), F.lcp.get(), tl.lmin.get(),
                           R.isa.get(), R.lcp.get(), tr.lmin.get(), lf, f, c_start.get(), c_pl.get());
        });
        std::vector<Run> got, want;
        for (u32 i = 0; i < n; i++)
            for (u32 o = 0; o < 2; o++) {
                u32 j = n;                          // the rule, by scanning
                for (u32 k = i + 1; k <= n; k++)
                    if (o ? F.isa[k] > F.isa[i] : F.isa[k] < F.isa[i]) {
                        j = k;
                        break;
                    }
                const u32 p = j - i;
                u32 start = 0;
                u64 pl = 0;
                if (j < n && text[i] == text[j]) {
                    u32 e = 0, b = 0;
                    while (j + e < n && text[i + e] == text[j + e]) e++;
                    while (b < i && text[i - 1 - b] == text[j - 1 - b]) b++;
                    if (b < p && b + e >= p && passes(f, p, b + p + e)) {
                        start = i - b;
                        pl = (u64)p << 32 | (b + p + e);
                    }
                    if (b >= p && b + e >= p) g_tie_broken++;
                }
                EXPECT(c_start[2 * (size_t)i + o] == start && c_pl[2 * (size_t)i + o] == pl);
                if (pl) got.push_back(Run(start, (u32)(pl >> 32), (u32)pl));
            }
        std::sort(got.begin(), got.end());
        for (const Run &r : all)
            if (passes(f, std::get<1>(r), std::get<2>(r))) want.push_back(r);
        EXPECT(got == want);                        // every run once, nothing else
        g_runs += got.size();
        g_positions += n;
    }
    const u32 at = lf == 2 ? 0 : 1;
    g_nlev[at] = std::max(g_nlev[at], ti.nlev);
    g_texts++;
}

// w x^k y z: the search from position 0 finds its first hit k + 1 positions away, whichever order needs it
static Bytes far_hit(u32 n, const char *wxyz) {
    Bytes t(n, (u8)wxyz[1]);
    t[0] = (u8)wxyz[0];
    if (n > 2) t[n - 2] = (u8)wxyz[2];
    if (n > 1) t[n - 1] = (u8)wxyz[3];
    return t;
}
// nine bytes in ten are `often`: more than half of all rows share their first byte, so a range minimum between two of them
// that lie far apart stays above 0 up to the top of the tree
static Bytes skewed(std::mt19937 &rng, u32 n, char often, char seldom) {
    Bytes t(n);
    for (u8 &b : t) b = (u8)(rng() % 10 ? often : seldom);
    return t;
}
// B^D A B^k A, D = TR_DIRECT (the bytes compared directly: the common prefix must reach them for a range minimum to be
// asked): position 0 sorts near the bottom of the rows that start with B^D, position D + 1 -- the next larger suffix -- at
// their top, and the minimum between the two rows is D: the range minimum goes over the whole tree
static Bytes far_min(u32 n) {
    Bytes t(n, 'B');
    if (n > TR_DIRECT) t[TR_DIRECT] = 'A';
    t[n - 1] = 'A';
    return t;
}
// (B^D A B^k)(B^D A B^k): the run of period D + 1 + k is found at position D with D bytes to its left, and in the reversed
// text the prefixes that end there -- B^D and B^(D+k) A B^D -- are the first and the last row that start with B^D: the same
// for the reversed text's range minimum
static Bytes far_min_back(u32 n) {
    const u32 k = n / 2 > TR_DIRECT + 1 ? n / 2 - TR_DIRECT - 1 : 0;
    Bytes u(TR_DIRECT + 1 + k, 'B');
    u[TR_DIRECT] = 'A';
    Bytes t = u;
    t.insert(t.end(), u.begin(), u.end());
    return t;
}
// u v u with a random u: the two copies are a run of period |u v|, and its two suffixes sort wherever u sorts
static Bytes far_rows(std::mt19937 &rng, u32 n) {
    const u32 half = n / 2;
    Bytes u = random_text(rng, half, 4), t = u;
    if (n & 1) t.push_back('N');
    t.insert(t.end(), u.begin(), u.end());
    return t;
}

int main() {
    std::mt19937 rng(0x7a9d);
    for (u32 lf : {2u, 6u}) {
        memset(tr_climbed, 0, sizeof tr_climbed);
        for (u32 n : {1u, 2u, 3u, 4u, 8u, 63u, 64u, 65u, 257u, 300u, 1100u, 2200u}) {
            check_text(Bytes(n, 'A'), lf);
            for (u32 p : {2u, 3u, 7u}) {
                Bytes t = periodic(n, p);
                check_text(t, lf);
                for (u32 k = 0; k < 3 && n > 8; k++) t[rng() % n] = (u8)("ACGT"[rng() % 4]);
                check_text(t, lf);
            }
            check_text(fibonacci(n), lf);
            for (u32 sigma : {1u, 2u, 4u, 256u}) check_text(random_text(rng, n, sigma), lf);
            check_text(far_hit(n, "ABBA"), lf);     // A^(n-1) then a smaller end: order 0 from every position to the end
            check_text(far_hit(n, "ABCC"), lf);
            check_text(far_hit(n, "CBAD"), lf);     // order 1 from position 0 to the last byte
            check_text(far_hit(n, "BAAC"), lf);
            check_text(far_rows(rng, n), lf);
            check_text(far_min(n), lf);
            check_text(skewed(rng, n, 'B', 'A'), lf);
            check_text(skewed(rng, n, 'A', 'B'), lf);
            if (n > 1100) continue;
            Bytes twice = random_text(rng, n, 4);   // a text followed by its own copy: one run over everything
            twice.insert(twice.end(), twice.begin(), twice.end());
            check_text(twice, lf);
            twice.back() = 'Z';
            check_text(twice, lf);
        }
        // (a range minimum moves its right end down by one group per level: it sees the top of a fan-out-4 tree of five
        // levels only from 2388 rows on)
        check_text(far_min(2600), lf);
        check_text(far_min_back(2600), lf);
        for (u32 kind = 0; kind < 4; kind++) {
            u32 top = 0;
            for (u32 lev = 0; lev <= FM_MS_MAXLEV; lev++)
                if (tr_climbed[kind][lev]) top = lev;
            g_top[(lf == 2 ? 0 : 4) + kind] = top;
            if (lf == 2)                            // every level of the deepest fan-out-4 tree, by every one of the four
                for (u32 lev = 0; lev <= g_nlev[0]; lev++) {
                    if (!tr_climbed[kind][lev]) std::fprintf(stderr, "climb %u never reached level %u of %u\n", kind, lev, g_nlev[0]);
                    EXPECT(tr_climbed[kind][lev] > 0);
                }
        }
    }
    EXPECT(g_runs > 0 && g_tie_broken > 0);
    std::printf("ok: the runs of %llu texts, %llu positions: %llu runs, %llu candidates dropped for a root further left\n",
                (unsigned long long)g_texts, (unsigned long long)g_positions, (unsigned long long)g_runs,
                (unsigned long long)g_tie_broken);
    std::printf("every tree level reached at fan-out 4 (%u levels): searches %u %u, range minima %u %u; at fan-out 64 (%u): %u %u, %u %u\n",
                g_nlev[0], g_top[0], g_top[1], g_top[2], g_top[3], g_nlev[1], g_top[4], g_top[5], g_top[6], g_top[7]);
    return 0;
}
