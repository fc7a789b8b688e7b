// Stand-alone host check of the palindrome kernel (csrc/tc_pal.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/pal_kernels.cpp -o pal_kernels && ./pal_kernels
// TC_FM_MS_HOST_CHECK compiles pal_centre_kernel and the range minimum of csrc/tc_lz.hpp it calls as plain C++, as
// host/check/tr_kernels.cpp does for the tandem-repeat kernel: the HIP keywords defined away, a workgroup of one lane, the
// lanes of a grid run one after another.  Everything is built naively -- the joint text S = text . sigma(reverse(text)),
// its suffixes sorted directly, the LCP array by comparing neighbours, the inverse array by scatter, the min tree by
// fm_lmin_kernel level over level at fan-outs 4 and 64 -- in heap blocks of exactly the entries the library's arrays hold,
// so a read one element outside any of them stops the run.  Every centre's word, for the budgets 0, 1, 3 and 16 and under
// the identity and the DNA complement, is compared with brute force: the pairs of the centre walked outwards, the mismatches
// counted, the last matching pair within the budget remembered.  Texts: unary, periodic, Fibonacci, random over 1, 2, 4 and
// 256 letters, random DNA with planted hairpins that carry substitutions, and texts that are one palindrome as a whole.
// The program asserts what no device test can see: at fan-out 4 the range minimum reached every level of the tree, the
// clamp cut a range minimum and ended a direct compare, some lane used all m + 1 turns, some lane dropped a trailing
// mismatch, and both the direct compare and the range minimum decided extensions.  The joint-text, count, fill and
// longest kernels need a workgroup's scan or atomics: they are checked on the device only.

#define TC_FM_MS_HOST_CHECK
#include "tc_pal.hpp"
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

static u8 g_sigma[2][256];      // [0: the identity, 1: the DNA complement]

// the word of centre c by walking its pairs outwards
static u64 brute_word(const Bytes &t, const u8 *sigma, u32 c, u32 m, u32 min_len) {
    const u32 n = (u32)t.size(), l0 = c / 2, r0 = (c + 1) / 2, bound = std::min(l0 + 1, n - r0);
    u32 best = 0, best_mm = 0, mm = 0;
    for (u32 k = 0; k < bound && mm <= m; k++) {
        if (t[l0 - k] != sigma[t[r0 + k]]) mm++;
        else best = k + 1, best_mm = mm;
    }
    const u32 len = 2 * best - 1 + (c & 1);
    return best && len >= min_len ? (u64)len << 32 | best_mm : 0;
}

static u64 g_texts = 0, g_centres = 0, g_found = 0;
static u32 g_nlev[2] = {}, g_top[2] = {};      // [fan-out 4, fan-out 64] the deepest tree, the highest level a range minimum reached
static void check_text(const Bytes &text, u32 lf) {
    const u32 n = (u32)text.size(), n2 = 2 * n, N = n2 + 1;
    if (!n) return;
    for (u32 which = 0; which < 2; which++) {
        const u8 *sigma = g_sigma[which];
        Bytes S(n2);
        for (u32 k = 0; k < n; k++) S[k] = text[k], S[n + k] = sigma[text[n - 1 - k]];
        Esa E;
        build_esa(E, S);
        const MinTree tl = min_tree_of(E.lcp.get(), N, lf);
        auto s_blk = block<u8>(n2);
        std::copy(S.begin(), S.end(), s_blk.get());
        auto word = block<u64>(n2 - 1);
        for (u32 m : {0u, 1u, 3u, 16u})
            for (u32 min_len : {1u, 4u}) {
                for (u32 c = 0; c + 1 < n2; c++) word[c] = ~0ull;
                launch(n2 - 1, [&] { pal_centre_kernel(s_blk.get(), n, E.isa.get(), E.lcp.get(), tl.lmin.get(), lf, m, min_len, word.get()); });
                for (u32 c = 0; c + 1 < n2; c++) {
                    const u64 want = brute_word(text, sigma, c, m, min_len);
                    if (word[c] != want)
                        std::fprintf(stderr, "n %u sigma %u m %u min_len %u centre %u: got %llx, want %llx\n", n, which, m, min_len, c,
                                     (unsigned long long)word[c], (unsigned long long)want);
                    EXPECT(word[c] == want);
                    g_found += want != 0;
                }
                g_centres += n2 - 1;
            }
        const u32 at = lf == 2 ? 0 : 1;
        g_nlev[at] = std::max(g_nlev[at], tl.nlev);
    }
    g_texts++;
}

// w . sigma(reverse(w)), with an odd length's middle byte between: the whole text is one palindrome
static Bytes whole(std::mt19937 &rng, u32 n, const u8 *sigma) {
    Bytes t = random_text(rng, n, 4);
    for (u32 k = 0; k < n / 2; k++) t[n - 1 - k] = sigma[t[k]];
    return t;
}
// random DNA with hairpins written over it: stems of 3 .. 40 pairs around a loop of 0 .. 3 bytes, 0 .. 3 substitutions in
// the right arm -- the first of them next to the loop, the second at the outer edge --, one stem at position 0 and one that
// ends at n - 1
static Bytes hairpins(std::mt19937 &rng, u32 n, const u8 *sigma) {
    Bytes t = random_text(rng, n, 4);
    for (u32 j = 0; j < 8 && n >= 16; j++) {
        const u32 stem = 3 + rng() % std::min(38u, n / 2 - 4), loop = rng() % 4, len = 2 * stem + loop;
        if (len > n) continue;
        const u32 s = j == 0 ? 0 : j == 1 ? n - len : rng() % (n - len + 1);
        for (u32 k = 0; k < stem; k++) t[s + len - 1 - k] = sigma[t[s + k]];
        for (u32 e = 0; e < j % 4; e++) {
            const u32 k = e == 0 ? stem - 1 : e == 1 ? 0 : rng() % stem;
            u8 &b = t[s + len - 1 - k];
            b = (u8)(b == 'A' ? 'C' : 'A');
        }
    }
    return t;
}

int main() {
    for (u32 x = 0; x < 256; x++) g_sigma[0][x] = g_sigma[1][x] = (u8)x;
    for (const char *p : {"AT", "CG", "at", "cg"}) g_sigma[1][(u8)p[0]] = (u8)p[1], g_sigma[1][(u8)p[1]] = (u8)p[0];
    std::mt19937 rng(0x9a11);
    for (u32 lf : {2u, 6u}) {
        memset(lz_climbed, 0, sizeof lz_climbed);
        for (u32 n : {1u, 2u, 3u, 4u, 5u, 8u, 9u, 31u, 32u, 33u, 64u, 257u, 700u}) {
            check_text(Bytes(n, 'A'), lf);
            check_text(Bytes(n, 'N'), lf);
            for (u32 p : {2u, 3u, 7u}) {
                Bytes t = periodic(n, p);
                check_text(t, lf);
                for (u32 k = 0; k < 3 && n > 8; k++) t[rng() % n] = (u8)("ACGT"[rng() % 4]);
                check_text(t, lf);
            }
            check_text(fibonacci(n), lf);
            for (u32 sigma : {1u, 2u, 4u, 256u}) check_text(random_text(rng, n, sigma), lf);
            for (u32 which = 0; which < 2; which++) {
                check_text(whole(rng, n, g_sigma[which]), lf);
                check_text(hairpins(rng, n, g_sigma[which]), lf);
            }
        }
        // (a range minimum moves its right end down by one group per level: it sees the top of a fan-out-4 tree of five
        // levels only from 2388 rows on -- a unary text of 1300 bytes, whose centres near either end ask the minimum between
        // two rows at opposite ends of the array)
        check_text(Bytes(1300, 'N'), lf);
        const u32 at = lf == 2 ? 0 : 1;
        for (u32 lev = 0; lev <= FM_MS_MAXLEV; lev++)
            if (lz_climbed[lev]) g_top[at] = lev;
        if (lf == 2)
            for (u32 lev = 0; lev <= g_nlev[0]; lev++) {
                if (!lz_climbed[lev]) std::fprintf(stderr, "no range minimum reached level %u of %u\n", lev, g_nlev[0]);
                EXPECT(lz_climbed[lev] > 0);
            }
    }
    for (u32 k = 0; k < 6; k++) {
        if (!pal_seen[k]) std::fprintf(stderr, "path %u never taken\n", k);
        EXPECT(pal_seen[k] > 0);
    }
    EXPECT(g_found > 0);
    std::printf("ok: the palindromes of %llu texts, %llu centres: %llu found\n", (unsigned long long)g_texts,
                (unsigned long long)g_centres, (unsigned long long)g_found);
    std::printf("clamp cut %llu range minima and ended %llu direct compares; %llu lanes used every turn, %llu dropped a trailing "
                "mismatch; extensions decided directly %llu, by a range minimum %llu\n",
                (unsigned long long)pal_seen[0], (unsigned long long)pal_seen[1], (unsigned long long)pal_seen[2],
                (unsigned long long)pal_seen[3], (unsigned long long)pal_seen[4], (unsigned long long)pal_seen[5]);
    std::printf("every tree level reached at fan-out 4 (%u levels): range minima %u; at fan-out 64 (%u): %u\n", g_nlev[0], g_top[0],
                g_nlev[1], g_top[1]);
    return 0;
}
