// Stand-alone host check of the unique-substring lanes (csrc/tc_sus.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/sus_kernels.cpp -o sus_kernels && ./sus_kernels
// TC_FM_MS_HOST_CHECK compiles sus_prefix_lane, sus_mark_lane and sus_point_lane, the range minimum of csrc/tc_lz.hpp and
// the row search of csrc/tc_fm_ms.hpp as plain C++, as host/check/maw_kernels.cpp does for the absent words: the HIP keywords
// defined away, the lanes run one after another.  Everything around them is built naively, the suffix array, the LCP array and the
// tree by check_common.hpp and check_esa.hpp -- suffixes sorted directly,
// the LCP array by comparing neighbours, the two scans by running loops, the min tree by fm_lmin_kernel level over level at
// fan-outs 4 and 64 -- in heap blocks of exactly the entries the library's arrays hold, so a read or a store one element
// outside any of them stops the run.  Every up, every MUS and every point answer is compared with brute force: the longest
// common prefix of every pair of suffixes (up[i] = 1 + the longest one of suffix i, where that many bytes are left), the MUS as
// the unique substrings whose two maximal proper factors are not unique, the point answer as the best of all unique substrings
// over the position; on the texts of at most 24 bytes these are in turn held against counts of every substring.  Texts: unary,
// periodic (2, 3, 7), Fibonacci, random over 1, 2, 4 and 200 letters, a text followed by its copy, a long MUS with a short one
// at its end (the leftmost search climbs to the top of the tree), and the staircase: many MUS over one position, the shortest
// in the middle.  The kernels around the lanes need a workgroup: they are checked on the device only.
#include <map>

#define TC_FM_MS_HOST_CHECK
#include "tc_sus.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

struct Pair {
    u32 s, len;
    bool operator==(const Pair &o) const { return s == o.s && len == o.len; }
};

// ---- brute force ---------------------------------------------------------------------------------------------------------
// up[i] = 1 + the longest common prefix of suffix i with any other suffix, 0 where that reaches the end of the text
static std::vector<u32> brute_up(const Bytes &t) {
    const u32 n = (u32)t.size();
    std::vector<u32> longest(n, 0), below(n + 1, 0), row(n + 1, 0);
    for (u32 i = n; i-- > 0;) {             // row[j] = the common prefix of suffixes i and j, from that of i + 1 and j + 1
        for (u32 j = 0; j < n; j++) row[j] = t[i] == t[j] ? below[j + 1] + 1u : 0u;
        row[n] = 0;
        for (u32 j = 0; j < n; j++)
            if (j != i) longest[i] = std::max(longest[i], row[j]);
        below.swap(row);
    }
    std::vector<u32> up(n);
    for (u32 i = 0; i < n; i++) up[i] = i + longest[i] < n ? longest[i] + 1u : 0u;
    return up;
}
// text[s .. s + l) is unique iff up[s] != 0 and l >= up[s]; "occurs at least twice" is "not unique", also for the empty string
static std::vector<Pair> brute_mus(const std::vector<u32> &up) {
    const u32 n = (u32)up.size();
    auto unique = [&](u32 s, u32 l) { return l != 0 && up[s] != 0 && l >= up[s]; };
    std::vector<Pair> out;
    for (u32 s = 0; s < n; s++)
        for (u32 l = 1; s + l <= n; l++)
            if (unique(s, l) && !unique(s, l - 1) && !(l > 1 && unique(s + 1, l - 1))) out.push_back(Pair{s, l});
    return out;
}
static std::vector<Pair> brute_point(const std::vector<u32> &up) {
    const u32 n = (u32)up.size();
    std::vector<Pair> out(n);
    for (u32 p = 0; p < n; p++) {
        u64 best = ~0ull;
        for (u32 s = 0; s <= p; s++) {
            if (!up[s]) continue;
            const u64 c = (u64)std::max(up[s], p - s + 1u) << 32 | s;
            best = std::min(best, c);
        }
        EXPECT(best != ~0ull);
        out[p] = Pair{(u32)best, (u32)(best >> 32)};
    }
    return out;
}
// the three again, from the counts of every substring (short texts)
static void by_counting(const Bytes &text, const std::vector<u32> &up, const std::vector<Pair> &mus, const std::vector<Pair> &point) {
    const std::string t(text.begin(), text.end());
    const u32 n = (u32)t.size();
    std::map<std::string, u32> cnt;
    for (u32 i = 0; i < n; i++)
        for (u32 l = 1; i + l <= n; l++) cnt[t.substr(i, l)]++;
    auto occ = [&](const std::string &w) { return w.empty() ? 2u : cnt[w]; };
    std::vector<Pair> m2;
    for (u32 i = 0; i < n; i++) {
        u32 u = 0;
        for (u32 l = 1; i + l <= n && !u; l++)
            if (cnt[t.substr(i, l)] == 1) u = l;
        EXPECT(u == up[i]);
        for (u32 l = 1; i + l <= n; l++) {
            const std::string w = t.substr(i, l);
            if (cnt[w] == 1 && occ(w.substr(1)) >= 2 && occ(w.substr(0, l - 1)) >= 2) m2.push_back(Pair{i, l});
        }
    }
    EXPECT(m2 == mus);
    for (u32 p = 0; p < n; p++) {
        u64 best = ~0ull;
        for (u32 s = 0; s <= p; s++)
            for (u32 l = p - s + 1; s + l <= n; l++)
                if (cnt[t.substr(s, l)] == 1) {
                    best = std::min(best, (u64)l << 32 | s);
                    break;
                }
        EXPECT(best == ((u64)point[p].len << 32 | point[p].s));
    }
}

static u64 g_texts = 0, g_positions = 0, g_mus = 0, g_counted = 0;
static u64 g_min_reached[FM_MS_MAXLEV + 1] = {}, g_search_reached[FM_MS_MAXLEV + 1] = {};
static u32 g_maxlev4 = 0;
static u64 g_tie_left = 0, g_interior = 0, g_uncovered = 0, g_up0 = 0, g_first = 0, g_last = 0, g_deep = 0;

static void check_text(const Bytes &text, u32 lf) {
    const u32 n = (u32)text.size(), N = n + 1;
    // the enhanced suffix array, naively
    const std::vector<u32> order = sort_suffixes(text);
    auto sa = block_of(order), lcp = block_of(lcp_of(text, order));
    // up: one lane per row, every entry written exactly once
    auto up = block<u32>(n);
    for (u32 i = 0; i < n; i++) up[i] = 0xdeadbeefu;
    for (u32 r = 0; r < N; r++) sus_prefix_lane(sa.get(), lcp.get(), N, r, up.get());
    const std::vector<u32> want_up = brute_up(text);
    for (u32 i = 0; i < n; i++) EXPECT(up[i] == want_up[i]);
    // the mark pass: mlen and endof, then the list from the same rule
    auto mlen = block<u32>(n), pred = block<u32>(n), nxt = block<u32>(N);
    for (u32 i = 0; i < n; i++) pred[i] = 0;
    std::vector<Pair> mus;
    for (u32 s = 0; s < n; s++) {
        const u32 v = s + 1 < n ? up[s + 1] : 0u;
        sus_mark_lane(n, s, up[s], v, mlen.get(), pred.get());
        if (sus_mus_rule(up[s], v)) mus.push_back(Pair{s, up[s]});
        EXPECT((mlen[s] != SUS_NONE) == sus_mus_rule(up[s], v));
    }
    const std::vector<Pair> want_mus = brute_mus(want_up);
    EXPECT(mus == want_mus);
    EXPECT(!mus.empty() && mus.size() <= n);
    for (size_t k = 0; k < mus.size(); k++) {
        EXPECT(pred[mus[k].s + mus[k].len - 1] == mus[k].s + 1);
        if (k) EXPECT(mus[k].s > mus[k - 1].s && mus[k].s + mus[k].len > mus[k - 1].s + mus[k - 1].len);
    }
    // the two scans
    for (u32 p = 1; p < n; p++) pred[p] = std::max(pred[p], pred[p - 1]);
    nxt[n] = n;
    for (u32 p = n; p-- > 0;) nxt[p] = mlen[p] != SUS_NONE ? p : nxt[p + 1];
    // the min tree over mlen
    const MinTree tree = min_tree_of(mlen.get(), n, lf);
    const u32 nlev = tree.nlev;
    const FmMsTree T = tree.view(mlen.get());
    // one lane per position
    const std::vector<Pair> want = brute_point(want_up);
    memset(lz_climbed, 0, sizeof lz_climbed);
    memset(fm_ms_climbed, 0, sizeof fm_ms_climbed);
    for (u32 p = 0; p < n; p++) {
        const u64 seen4 = sus_seen[4];
        const u64 got = sus_point_lane(T, pred.get(), nxt.get(), n, p);
        EXPECT((u32)got == want[p].s && (u32)(got >> 32) == want[p].len);
        EXPECT(want[p].s <= p && p < want[p].s + want[p].len && want_up[want[p].s] != 0 && want[p].len >= want_up[want[p].s]);
        if (p) EXPECT(want[p].len + 1 >= want[p - 1].len && want[p - 1].len + 1 >= want[p].len);
        // what the covering MUS look like here
        u32 covering = 0, shortest = SUS_NONE, times = 0, first_at = 0, k_first = 0, k_last = 0;
        for (u32 k = 0; k < mus.size(); k++) {
            if (mus[k].s > p || mus[k].s + mus[k].len <= p) continue;
            if (!covering) k_first = k;
            k_last = k;
            covering++;
            if (mus[k].len < shortest) {
                shortest = mus[k].len;
                times = 0;
                first_at = k;
            }
            if (mus[k].len == shortest) times++;
        }
        EXPECT((covering == 0) == (sus_seen[4] != seen4));
        if (!covering) g_uncovered++;
        const bool by_cover = covering && want[p].len == shortest && want[p].s == mus[first_at].s;
        if (by_cover && times > 1) g_tie_left++;
        if (by_cover && first_at != k_first && first_at != k_last) g_interior++;
        if (covering > 16) g_deep++;     // (more than the square of the small fan-out)
        if (want_up[p] == 0) g_up0++;
        if (p == 0) g_first++;
        if (p == n - 1) g_last++;
    }
    if (lf == 2) {
        for (u32 v = 0; v <= FM_MS_MAXLEV; v++) {
            g_min_reached[v] += lz_climbed[v];
            g_search_reached[v] += fm_ms_climbed[1][v];
        }
        g_maxlev4 = std::max(g_maxlev4, nlev);
    }
    if (n <= 24) {
        by_counting(text, want_up, want_mus, want);
        g_counted++;
    }
    g_texts++;
    g_positions += n;
    g_mus += mus.size();
}

static void append(Bytes &t, const Bytes &x) { t.insert(t.end(), x.begin(), x.end()); }
// a Y b . Y b q . a Y q: the MUS (0, |Y| + 2) and, at its last byte, the MUS b Y[0] of length 2 -- nothing starts between them
static Bytes long_then_short(std::mt19937 &rng, u32 m) {
    const Bytes Y = random_text(rng, m, 4);
    Bytes t{'a'};
    append(t, Y); t.push_back('b');
    append(t, Y); t.push_back('b'); t.push_back('q'); t.push_back('a');
    append(t, Y); t.push_back('q');
    return t;
}
// A, then per step a separator byte and a copy of a stretch of A that starts `stride` further right and whose length wanders
static Bytes staircase(std::mt19937 &rng, u32 base, u32 steps, u32 stride) {
    const Bytes A = random_text(rng, 2 * base + steps * stride + 8, 4);
    Bytes t = A;
    u32 ln = base + steps;
    for (u32 k = 0; k < steps; k++) {
        if (k) ln = std::max<int>((int)base, (int)ln + (int)(rng() % (2 * stride - 1)) - (int)(stride - 1));
        ln = std::min<u32>(ln, (u32)A.size() - k * stride);
        t.push_back((u8)(128 + k % 100));
        t.insert(t.end(), A.begin() + k * stride, A.begin() + k * stride + ln);
    }
    t.push_back(255);
    return t;
}

int main() {
    std::mt19937 rng(0x5051);
    for (u32 lf : {2u, 6u}) {
        for (u32 n : {1u, 2u, 3u, 5u, 8u, 13u, 17u, 24u, 40u, 63u, 64u, 65u, 257u, 300u, 640u, 1100u, 2200u}) {
            check_text(Bytes(n, 'A'), lf);
            for (u32 p : {2u, 3u, 7u}) check_text(periodic(n, p), lf);
            check_text(fibonacci(n), lf);
            for (u32 sigma : {1u, 2u, 4u, 200u}) check_text(random_text(rng, n, sigma), lf);
            if (n > 1100) continue;
            Bytes twice = random_text(rng, n, 4);   // a text followed by its own copy; a text whose last byte is new
            append(twice, twice);
            check_text(twice, lf);
            twice.back() = 'Z';
            check_text(twice, lf);
        }
        check_text(Bytes(4096, 'A'), lf);           // one MUS over every position: the range minimum spans the whole top level
        const u64 searched = sus_seen[3];
        for (u32 m : {5u, 300u, 1100u}) check_text(long_then_short(rng, m), lf);
        EXPECT(sus_seen[3] > searched);
        const u64 deep = g_deep, inner = g_interior, ties = g_tie_left;
        check_text(staircase(rng, 44, 40, 2), lf);
        EXPECT(g_deep > deep && g_interior > inner && g_tie_left > ties);
    }
    for (u32 v = 0; v <= g_maxlev4; v++) EXPECT(g_min_reached[v] > 0 && g_search_reached[v] > 0);   // every level of the fan-out-4 tree
    EXPECT(g_maxlev4 >= 5);
    EXPECT(sus_seen[0] > 0 && sus_seen[1] > 0 && sus_seen[2] > 0);     // an answer of each of the three kinds
    EXPECT(sus_seen[5] > 0);        // two candidates of one length: the start decided
    EXPECT(g_tie_left > 0);         // a tie among the covering MUS, resolved to the left
    EXPECT(g_interior > 0);         // the shortest covering MUS neither the first nor the last of them
    EXPECT(g_uncovered > 0);        // a position no MUS covers
    EXPECT(g_up0 > 0);              // positions with up = 0
    EXPECT(g_first > 0 && g_last > 0 && g_counted > 0);
    std::printf("ok: the unique substrings of %llu texts, %llu positions, %llu MUS, %llu texts held against substring counts; "
                "every tree level reached at fan-out 4 (%u levels) by the range minimum and by the leftmost search\n",
                (unsigned long long)g_texts, (unsigned long long)g_positions, (unsigned long long)g_mus,
                (unsigned long long)g_counted, g_maxlev4);
    return 0;
}
