// Stand-alone host check of the minimal-absent-word lanes (csrc/tc_maw.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/maw_kernels.cpp -o maw_kernels && ./maw_kernels
// TC_FM_MS_HOST_CHECK compiles maw_row_body (both set widths), maw_range_or and the two row searches of csrc/tc_fm_ms.hpp
// as plain C++, as host/check/rep_kernels.cpp does for the repeats: the HIP keywords defined away, the lanes run one after
// another.  Everything is built naively -- suffixes sorted directly, the LCP array by comparing neighbours, the last
// column from the text, the change counts by a running sum, the min tree by fm_lmin_kernel and the OR tree by plain loops,
// level over level at fan-outs 4 and 64 -- in heap blocks of exactly the entries the library's arrays hold, so a read one
// element outside any of them stops the run.  Every row's words, in order, under several length windows, are compared with
// what one stack walk over the LCP array says: the walk closes every LCP interval and the root, finds the children by
// scanning for the boundaries, collects the left bytes of the node and of every child directly and books the words at the
// child's boundary row.  On the texts of at most 40 bytes the walk's words are in turn compared with the definition: every
// word u . b, u a substring, that does not occur while its two maximal proper factors do.  Texts: unary, periodic (2, 3, 7),
// Fibonacci, random over 1, 2, 4, 64, 65 and 256 letters, a text followed by its copy, lengths 1 .. 2200 (and one of 2600,
// the shortest at which a range OR climbs to the top of a five-level tree), each of the 256 bytes once.  The tree build and
// the kernel around the body need a workgroup: they are checked on the device only.
#include <set>

#define TC_FM_MS_HOST_CHECK
#include "tc_maw.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

struct Word {
    u32 a, pos, len;
    bool operator==(const Word &o) const { return a == o.a && pos == o.pos && len == o.len; }
};

// ---- the enhanced suffix array of a text, naively, in blocks of the library's sizes --------------------------------------
struct Esa {
    u32 n = 0, N = 0, primary = 0;
    std::vector<int> left;                      // -1: Nothing; left[0] = the text's last byte
    std::unique_ptr<u32[]> sa, lcp;
    std::unique_ptr<u8[]> L;
    std::unique_ptr<u64[]> chg;
    u64 alpha[4] = {};
    u32 sigma = 0;
};
static void build_esa(Esa &e, const Bytes &text) {
    const u32 n = e.n = (u32)text.size(), N = e.N = n + 1;
    const std::vector<u32> sa = sort_suffixes(text);
    e.sa = block_of(sa);
    e.lcp = block_of(lcp_of(text, sa));
    e.L = block<u8>(N);
    e.chg = block<u64>(N);
    e.left.assign(N, -1);
    for (u8 b : text) e.alpha[b >> 6] |= 1ull << (b & 63);
    for (u32 i = 0; i < 4; i++) e.sigma += (u32)__builtin_popcountll(e.alpha[i]);
    for (u32 j = 0; j < N; j++) {
        if (e.sa[j] == 0) e.primary = j;
        e.left[j] = e.sa[j] ? (int)text[e.sa[j] - 1] : -1;
        e.L[j] = e.sa[j] ? text[e.sa[j] - 1] : (u8)0;             // the sentinel slot holds byte 0, as sa_build writes it
        e.chg[j] = j ? e.chg[j - 1] + (e.left[j] != e.left[j - 1] ? 1u : 0u) : 0u;
    }
}

// ---- what the stack walk says: want[k] = the words of the boundary row k, in order -----------------------------------------
static std::vector<std::vector<Word>> by_stack_walk(const Esa &e, u32 min_len, u32 max_len) {
    std::vector<std::vector<Word>> want(e.N);
    auto close = [&](u32 l, u32 lb, u32 rb) {
        if (l + 2 < min_len || (max_len && l + 2 > max_len)) return;
        bool lw[256] = {};
        for (u32 r = lb; r <= rb; r++)
            if (e.left[r] >= 0) lw[e.left[r]] = true;
        u32 cl = lb;
        bool is_first = true;
        for (u32 r = lb + 1; r <= rb + 1; r++) {
            if (r <= rb && e.lcp[r] != l) continue;
            // the child [cl, r - 1]; its words go to the boundary row that starts it, the first child's to the first boundary
            const u32 cr = r - 1;
            if (!(is_first && e.sa[cl] + l == e.n)) {
                bool lc[256] = {};
                for (u32 x = cl; x <= cr; x++)
                    if (e.left[x] >= 0) lc[e.left[x]] = true;
                u32 row = cl;
                if (is_first) {
                    row = lb + 1;
                    while (e.lcp[row] != l) row++;
                }
                for (u32 a = 0; a < 256; a++)
                    if (lw[a] && !lc[a]) want[row].push_back(Word{a, e.sa[cl], l + 2});
            }
            is_first = false;
            cl = r;
        }
    };
    struct Open { u32 l, lb; };
    std::vector<Open> stack{{0, 0}};
    for (u32 r = 1; r <= e.N; r++) {
        const u32 v = r < e.N ? e.lcp[r] : 0;
        u32 lb = r - 1;
        while (stack.back().l > v) {
            const Open o = stack.back();
            stack.pop_back();
            lb = o.lb;
            close(o.l, o.lb, r - 1);
        }
        if (stack.back().l < v) stack.push_back({v, lb});
    }
    if (e.N > 1) close(0, 0, e.N - 1);         // the root
    return want;
}

// ---- the definition, for short texts -------------------------------------------------------------------------------------
static std::set<std::string> by_definition(const Bytes &text) {
    const std::string t(text.begin(), text.end());
    std::set<std::string> subs, out;
    for (size_t i = 0; i < t.size(); i++)
        for (size_t l = 1; i + l <= t.size(); l++) subs.insert(t.substr(i, l));
    for (const std::string &u : subs)
        for (int b = 0; b < 256; b++) {
            const std::string x = u + (char)b;
            if (!subs.count(x) && subs.count(x.substr(1))) out.insert(x);
        }
    return out;
}

static u64 g_texts = 0, g_rows = 0, g_words = 0, g_defined = 0, g_wide = 0, g_reached[2][FM_MS_MAXLEV + 1] = {};
static u32 g_maxlev[2] = {};

template <bool WIDE>
static void run_rows(const Esa &e, const MawArgs &P, const FmMsTree &T, const MawTree &O, const u8 *byte_of,
                     const std::vector<std::vector<Word>> &want) {
    for (u32 k = 1; k < e.N; k++) {
        std::vector<Word> got;
        const u32 c = maw_row_body<WIDE>(P, T, O, k, [&](u32 at, u32 cl, MawSet<WIDE> d) {
            EXPECT(at == got.size());
            for (u32 i = 0; i < MAW_WORDS; i++)
                for (u32 b = 0; b < 64; b++)
                    if (d.w[i] >> b & 1) got.push_back(Word{WIDE ? 64 * i + b : (u32)byte_of[b], e.sa[cl], e.lcp[k] + 2});
        });
        EXPECT(c == got.size() && c <= 512);
        EXPECT(got == want[k]);
        g_words += c;
    }
    g_rows += e.N;
}

static void check_text(const Bytes &text, u32 lf) {
    Esa e;
    build_esa(e, text);
    const u32 N = e.N;
    const MinTree tree = min_tree_of(e.lcp.get(), N, lf);
    const u32 *off = tree.off, *lmin = tree.lmin.get();
    const u32 nlev = tree.nlev, words = tree.words;
    u8 code_of[256] = {}, byte_of[64] = {};
    for (u32 v = 0; v < 256; v++) {
        code_of[v] = (u8)maw_code_of(e.alpha, v);
        if (e.alpha[v >> 6] >> (v & 63) & 1) byte_of[code_of[v] & 63] = (u8)v;
    }
    const FmMsTree T = tree.view(e.lcp.get());
    const u32 windows[][2] = {{2, 0}, {2, 2}, {3, 0}, {3, 5}, {2, 16}, {20, 0}};
    for (int wide = e.sigma <= 64 ? 0 : 1; wide < 2; wide++) {     // (a small alphabet runs under both widths)
        // the OR tree by plain loops: level 1 from the left bytes, every further level from the one below
        const u32 W = wide ? 4 : 1;
        auto ortree = block<u64>((size_t)words * W);
        for (size_t i = 0; i < (size_t)words * W; i++) ortree[i] = 0;
        for (u32 r = 0; r < N; r++) {
            if (e.left[r] < 0) continue;
            const u32 c = wide ? (u32)e.left[r] : code_of[e.left[r]];
            for (u32 k = 1, j = r >> lf; k <= nlev; k++, j >>= lf) ortree[((size_t)off[k] + j) * W + (c >> 6)] |= 1ull << (c & 63);
        }
        MawTree O;
        O.L = e.L.get(); O.ortree = ortree.get(); O.s_off = off; O.s_code = code_of; O.N = N; O.lf = lf; O.primary = e.primary;
        for (const auto &w : windows) {
            MawArgs P;
            P.lcp = e.lcp.get(); P.lmin = lmin; P.sa = e.sa.get(); P.chg = e.chg.get(); P.L = e.L.get();
            P.ortree = ortree.get(); P.N = N; P.lf = lf; P.primary = e.primary; P.min_len = w[0]; P.max_len = w[1];
            for (u32 i = 0; i < 4; i++) P.alpha[i] = e.alpha[i];
            const std::vector<std::vector<Word>> want = by_stack_walk(e, w[0], w[1]);
            EXPECT(want[0].empty());
            memset(maw_or_level, 0, sizeof maw_or_level);
            if (wide) run_rows<true>(e, P, T, O, byte_of, want);
            else run_rows<false>(e, P, T, O, byte_of, want);
            for (u32 v = 0; v <= FM_MS_MAXLEV; v++) g_reached[lf == 2 ? 0 : 1][v] += maw_or_level[v];
            if (w[0] == 2 && w[1] == 0 && !wide && e.n <= 40) {    // the walk against the definition
                std::set<std::string> got;
                for (const auto &row : want)
                    for (const Word &x : row) {
                        std::string s(1, (char)x.a);
                        s.append(text.begin() + x.pos, text.begin() + x.pos + x.len - 1);
                        EXPECT(s.size() == x.len && got.insert(s).second);     // every word once
                    }
                EXPECT(got == by_definition(text));
                g_defined++;
            }
        }
        if (wide) g_wide++;
    }
    g_maxlev[lf == 2 ? 0 : 1] = std::max(g_maxlev[lf == 2 ? 0 : 1], nlev);
    g_texts++;
}

// above four letters the codes are spread over the whole byte range, 256 / sigma apart, so that the wide sets have members
// in all four words; sigma = 65 starts at byte 0
static Bytes spread_text(std::mt19937 &rng, u32 n, u32 sigma) {
    return random_text(rng, n, sigma > 4 ? byte_values(sigma == 65 ? 0 : 1, sigma, 256 / sigma) : letters("ACGT", sigma));
}

int main() {
    std::mt19937 rng(0x3a7);
    for (u32 lf : {2u, 6u}) {
        for (u32 n : {1u, 2u, 3u, 5u, 8u, 13u, 17u, 30u, 40u, 63u, 64u, 65u, 257u, 258u, 300u, 640u, 1100u, 2200u}) {
            check_text(Bytes(n, 'A'), lf);
            for (u32 p : {2u, 3u, 7u}) check_text(periodic(n, p), lf);
            check_text(fibonacci(n), lf);
            for (u32 sigma : {1u, 2u, 4u, 64u, 65u, 256u}) check_text(spread_text(rng, n, sigma), lf);
            if (n > 1100) continue;
            Bytes twice = random_text(rng, n, 4);   // a text followed by its own copy; a text whose last byte is new
            twice.insert(twice.end(), twice.begin(), twice.end());
            check_text(twice, lf);
            twice.back() = 'Z';
            check_text(twice, lf);
        }
        check_text(random_text(rng, 2600, 4), lf);
        Bytes all(256);                             // each byte once: 65 281 words of length 2, 256 children under the root
        for (u32 i = 0; i < 256; i++) all[i] = (u8)(i * 167u + 13u);
        const u64 before = g_words;
        check_text(all, lf);
        EXPECT(g_words - before == 65281u + 65281u + 0u + 0u + 65281u + 0u);   // the six windows: three of them hold length 2
    }
    for (u32 v = 0; v <= g_maxlev[0]; v++) EXPECT(g_reached[0][v] > 0);         // every level of the fan-out-4 tree
    EXPECT(g_maxlev[0] >= 5);
    EXPECT(maw_seen[0] > 0);        // the dropped first child
    EXPECT(maw_seen[1] > 0);        // a child of the primary row alone
    EXPECT(maw_seen[2] > 0);        // the chg exit
    EXPECT(maw_seen[3] > 0);        // the lb = k - 1 shortcut
    EXPECT(maw_seen[4] > 0);        // words for both children of one lane
    EXPECT(maw_seen[5] > 0);        // a wide set with members in all four words
    EXPECT(g_words > 0 && g_defined > 0 && g_wide > 0);
    std::printf("ok: the minimal absent words of %llu texts, %llu rows: %llu words, %llu texts held against the definition; "
                "every tree level reached at fan-out 4 (%u levels)\n", (unsigned long long)g_texts, (unsigned long long)g_rows,
                (unsigned long long)g_words, (unsigned long long)g_defined, g_maxlev[0]);
    return 0;
}
