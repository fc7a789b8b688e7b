// Stand-alone host check of the LPF kernel and its range minimum (csrc/tc_lz.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/lz_kernels.cpp -o lz_kernels && ./lz_kernels
// TC_FM_MS_HOST_CHECK compiles the bodies as plain C++, as host/check/fm_ms_kernels.cpp does for the row searches that
// the LPF kernel calls: the HIP keywords defined away, a workgroup of one lane, the lanes of a grid run one after another.
// Everything is built naively -- suffixes sorted directly, the LCP array by comparing neighbours, the two min trees
// (over the suffix array and over the LCP array) by fm_lmin_kernel level over level at fan-outs 4 and 64 -- in heap blocks
// of exactly the size the library allocates, so a read one element outside any of them stops the run.  What it walks:
//   - lz_range_min alone, on arrays no text has (all large, ascending, sparse small values, random), against a running
//     minimum, over all pairs of rows (every seventh upper end at the largest sizes): this is where every level of a
//     fan-out-4 tree is reached;
//   - lz_lpf_kernel, one lane per row, against brute force -- lpf[i] as the maximum over all j < i of a table of all
//     pairwise common prefixes, src[i] by the neighbour rule over the ranks of all j < i -- on unary, periodic (2, 3, 7),
//     Fibonacci and random texts over 1, 2, 4 and 256 letters, with n on both sides of a tree group.
// It asserts that the range minimum climbed to every level of a fan-out-4 tree of 4096 rows at least once.  The tile
// kernels of the parse and the rounds of the inverse need barriers between lanes: they are checked on the device only.

#define TC_FM_MS_HOST_CHECK
#include "tc_lz.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

// ---- a min tree over any u32 array, by the library's kernel ------------------------------------------------------------
struct Tree {
    u32 N = 0;
    std::unique_ptr<u32[]> base;
    MinTree min;
    FmMsTree view() const { return min.view(base.get()); }
};
static void build_tree(Tree &t, const std::vector<u32> &a, u32 lf) {
    t.N = (u32)a.size();
    t.base = block_of(a);
    t.min = min_tree_of(t.base.get(), t.N, lf);
    EXPECT(t.min.nlev >= 1 && t.min.cnt[t.min.nlev] <= (1u << lf) && t.min.cnt[0] == t.N);
}

// ---- 1: the range minimum alone ----------------------------------------------------------------------------------------
static u64 g_ranges = 0;
static void check_range_min(const std::vector<u32> &a, u32 lf, u32 hi_step) {
    Tree t;
    build_tree(t, a, lf);
    const FmMsTree T = t.view();
    for (u32 lo = 0; lo < t.N; lo++) {
        u32 m = 0xffffffffu, next = lo;
        for (u32 hi = lo; hi < t.N; hi++) {
            m = std::min(m, a[hi]);
            if (hi != next && hi != t.N - 1) continue;
            next = hi + hi_step;
            EXPECT(lz_range_min(T, lo, hi) == m);
            g_ranges++;
        }
    }
}
static void range_minima(std::mt19937 &rng) {
    for (u32 lf : {2u, 3u, 6u})
        for (u32 N : {1u, 2u, 3u, 4u, 5u, 16u, 17u, 63u, 64u, 65u, 255u, 257u, 1025u, 4096u, 4097u}) {
            if (lf == 3 && N > 300) continue;
            const u32 step = N > 300 ? 7 : 1;
            std::vector<u32> a(N, 9);                // all large: nothing ends a climb early
            check_range_min(a, lf, step);
            if (lf == 2 && N == 4096) {              // 1024, 256, 64, 16 and 4 entries: five tree levels, every one of them scanned
                u32 off[FM_MS_MAXLEV + 1], cnt[FM_MS_MAXLEV + 1], words;
                EXPECT(fm_ms_tree_shape(N, lf, off, cnt, &words) == 5);
                for (u32 l = 0; l <= 5; l++) EXPECT(lz_climbed[l] > 0);
            }
            std::vector<u32> b(N);                   // ascending from 1, as the LCP array of a unary text is
            for (u32 j = 0; j < N; j++) b[j] = j + 1;
            check_range_min(b, lf, step);
            std::vector<u32> c(N);                   // random small values
            for (u32 &v : c) v = rng() % 4;
            check_range_min(c, lf, step);
            std::vector<u32> d(N, 1000);             // a few small values far apart
            for (int k = 0; k < 3; k++) d[rng() % N] = 1 + rng() % 7;
            check_range_min(d, lf, step);
        }
}

// ---- 2: the LPF kernel ---------------------------------------------------------------------------------------------------
static u64 g_texts = 0, g_positions = 0;
static void check_lpf(const Bytes &text, u32 lf) {
    const u32 n = (u32)text.size(), N = n + 1;
    const std::vector<u32> sa = sort_suffixes(text), rank = inverse_of(sa);
    std::vector<u32> lcp(N, 0);
    // all pairwise common prefixes: cp[i][j] = lcp(i, j), from the end of the text
    std::vector<std::vector<u32>> cp(N, std::vector<u32>(N, 0));
    for (u32 i = n; i-- > 0;)
        for (u32 j = n; j-- > 0;) cp[i][j] = text[i] == text[j] ? cp[i + 1][j + 1] + 1 : 0;
    for (u32 j = 1; j < N; j++) lcp[j] = cp[sa[j - 1]][sa[j]];
    Tree ts, tl;
    build_tree(ts, sa, lf);
    build_tree(tl, lcp, lf);
    auto pack = block<u64>(n);
    for (u32 i = 0; i < n; i++) pack[i] = ~0ull;
    launch(n, [&] { lz_lpf_kernel(ts.base.get(), tl.base.get(), ts.min.lmin.get(), tl.min.lmin.get(), N, lf, pack.get()); });
    for (u32 i = 0; i < n; i++) {
        u32 best = 0, lo = N, hi = N;               // the maximum over all j < i; the two neighbours among them
        for (u32 j = 0; j < i; j++) {
            best = std::max(best, cp[i][j]);
            if (rank[j] < rank[i] && (lo == N || rank[j] > rank[lo])) lo = j;
            if (rank[j] > rank[i] && (hi == N || rank[j] < rank[hi])) hi = j;
        }
        const u32 llo = lo < N ? cp[i][lo] : 0, lhi = hi < N ? cp[i][hi] : 0;
        const u32 want_lpf = std::max(llo, lhi), want_src = want_lpf ? (llo >= lhi ? lo : hi) : 0;
        EXPECT(want_lpf == best);                   // the neighbour rule attains the maximum
        EXPECT((u32)pack[i] == want_lpf);
        EXPECT((u32)(pack[i] >> 32) == want_src);
    }
    g_texts++;
    g_positions += n;
}

int main() {
    std::mt19937 rng(0x7a11);
    range_minima(rng);
    for (u32 lf : {2u, 6u})
        for (u32 n : {1u, 2u, 3u, 62u, 63u, 64u, 65u, 300u, 1100u}) {
            check_lpf(Bytes(n, 'A'), lf);
            for (u32 p : {2u, 3u, 7u}) check_lpf(periodic(n, p), lf);
            check_lpf(fibonacci(n), lf);
            for (u32 sigma : {1u, 2u, 4u, 256u}) check_lpf(random_text(rng, n, sigma), lf);
            Bytes twice = random_text(rng, n, 4);   // a text followed by its own copy; a text whose last byte is new
            twice.insert(twice.end(), twice.begin(), twice.end());
            check_lpf(twice, lf);
            twice.back() = 'Z';
            check_lpf(twice, lf);
        }
    std::printf("ok: %llu range minima; the LPF array of %llu texts, %llu positions\n", (unsigned long long)g_ranges,
                (unsigned long long)g_texts, (unsigned long long)g_positions);
    return 0;
}
