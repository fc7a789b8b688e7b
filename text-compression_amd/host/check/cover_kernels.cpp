// Stand-alone host check of the repeat-cover lanes (csrc/tc_cov.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/cover_kernels.cpp -o cover_kernels && ./cover_kernels
// TC_FM_MS_HOST_CHECK compiles cov_seed_kernel (both instances), cov_reach and cov_lane_bits, the range minimum of
// csrc/tc_lz.hpp and the row searches of csrc/tc_fm_ms.hpp as plain C++, as host/check/sus_kernels.cpp does for the unique
// substrings: the HIP keywords defined away, the lanes run one after another.  Everything around them is built naively -- by
// check_common.hpp and check_esa.hpp the suffixes sorted directly, the LCP array by comparing neighbours, the two min trees by
// fm_lmin_kernel level over level at fan-outs 4 and 64; here the tiles' maxima, the spine and the scan inside a tile by running loops in the kernels' own geometry
// (COV_TILE positions per tile, COV_ITEMS in a row per lane) -- in heap blocks of exactly the entries the library's arrays hold,
// so a read or a store one element outside any of them stops the run.  Every seed is compared with a dictionary of the L-mers,
// every cover, span, mask and dedup with a difference array over the seeds; on the texts of at most 24 bytes the cover is in turn
// held against every substring of at least L bytes.  Texts: unary, periodic (2, 3, 7), Fibonacci, random over 1, 2, 4 and 200
// letters, a text followed by its copy, one letter and then 2600 times another; and the general form on arrays no text produces: all zero, one long entry, entries of
// 0xffffffff, random lengths.  The kernels around the lanes need a workgroup: they are checked on the device only.
#include <map>

#define TC_FM_MS_HOST_CHECK
#include "tc_cov.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

struct Span {
    u32 s, len;
    bool operator==(const Span &o) const { return s == o.s && len == o.len; }
};
struct Cover {
    std::vector<u8> cov;
    std::vector<Span> spans;
};

static u64 g_texts = 0, g_calls = 0, g_seeds = 0, g_arrays = 0, g_counted = 0, g_carried = 0, g_spans = 0;
static u64 g_down[FM_MS_MAXLEV + 1] = {}, g_up[FM_MS_MAXLEV + 1] = {}, g_min[FM_MS_MAXLEV + 1] = {};
static u32 g_maxlev4 = 0;

// ---- brute force ---------------------------------------------------------------------------------------------------------
static std::vector<u32> brute_seeds(const Bytes &t, u32 L, u32 q, bool later) {
    const u32 n = (u32)t.size();
    std::vector<u32> out;
    if (L > n) return out;
    std::map<std::string, std::vector<u32>> where;
    for (u32 i = 0; i + L <= n; i++) where[std::string(t.begin() + i, t.begin() + i + L)].push_back(i);
    for (auto &kv : where)
        if (kv.second.size() >= q) out.insert(out.end(), kv.second.begin() + (later ? 1 : 0), kv.second.end());
    std::sort(out.begin(), out.end());
    return out;
}
// the cover of an array of lengths, by a difference array
static Cover brute_cover_of_len(const std::vector<u32> &len, u32 L) {
    const u32 n = (u32)len.size();
    std::vector<int> d(n + 1, 0);
    for (u32 i = 0; i < n; i++) {
        if (len[i] < L) continue;
        d[i]++;
        d[(u32)std::min<u64>(n, (u64)i + len[i])]--;
    }
    Cover c;
    c.cov.assign(n, 0);
    int depth = 0;
    for (u32 p = 0; p < n; p++) {
        depth += d[p];
        c.cov[p] = depth > 0;
        if (c.cov[p] && (p == 0 || !c.cov[p - 1])) c.spans.push_back(Span{p, 0});
        if (c.cov[p]) c.spans.back().len++;
    }
    return c;
}
// every occurrence (LATER: but the leftmost) of every substring of at least L bytes that occurs at least q times
static std::vector<u8> brute_cover_by_substrings(const Bytes &t, u32 L, u32 q, bool later) {
    const u32 n = (u32)t.size();
    std::vector<u8> cov(n, 0);
    std::map<std::string, std::vector<u32>> where;
    for (u32 l = L; l <= n; l++)
        for (u32 i = 0; i + l <= n; i++) where[std::string(t.begin() + i, t.begin() + i + l)].push_back(i);
    for (auto &kv : where) {
        if (kv.second.size() < q) continue;
        for (size_t k = later ? 1 : 0; k < kv.second.size(); k++)
            for (u32 p = kv.second[k]; p < kv.second[k] + kv.first.size(); p++) cov[p] = 1;
    }
    return cov;
}

// ---- the core, in the kernels' geometry: len is a heap block of exactly n words ---------------------------------------------
static Cover run_core(const u32 *len, u32 n, u32 L) {
    const u32 tiles = (n + COV_TILE - 1) / COV_TILE;
    auto tmax = block<u32>(tiles);
    std::vector<u8> tile_counts(tiles, 0);
    for (u32 t = 0; t < tiles; t++) {               // cov_reduce_kernel
        u32 hi = 0;
        for (u64 i = (u64)t * COV_TILE; i < std::min<u64>(n, (u64)(t + 1) * COV_TILE); i++) {
            const u32 e = cov_reach(n, i, len[i], L);
            if (e) tile_counts[t] = 1;
            hi = std::max(hi, e);
        }
        tmax[t] = hi;
    }
    u32 run_tiles = 0;                              // cov_spine_kernel
    for (u32 t = 0; t < tiles; t++) {
        const u32 c = tmax[t];
        tmax[t] = run_tiles;
        run_tiles = std::max(run_tiles, c);
    }
    Cover out;
    out.cov.assign(n, 0);
    std::vector<u32> starts, ends;
    for (u32 t = 0; t < tiles; t++) {
        if (!tile_counts[t] && (u64)tmax[t] > (u64)t * COV_TILE) g_carried++;   // a tile without a position that counts, covered by the carry
        u32 run = tmax[t];
        for (u32 lane = 0; lane < COV_NT; lane++) {
            const u64 base = (u64)t * COV_TILE + (u64)lane * COV_ITEMS;
            u32 r[COV_ITEMS + 1];
            for (u32 k = 0; k <= COV_ITEMS; k++) r[k] = base + k < n ? cov_reach(n, base + k, len[base + k], L) : 0u;
            const CovBits b = cov_lane_bits(n, base, r, run);
            for (u32 k = 0; k < COV_ITEMS; k++) {
                if (base + k >= n) {
                    EXPECT(!((b.cov | b.st | b.en) >> k & 1u));
                    continue;
                }
                out.cov[base + k] = b.cov >> k & 1u;
                if (b.st >> k & 1u) starts.push_back((u32)(base + k));
                if (b.en >> k & 1u) ends.push_back((u32)(base + k));
                run = std::max(run, r[k]);          // (the wave scan and the LDS words of cov_tile_run)
            }
        }
    }
    EXPECT(starts.size() == ends.size());
    for (size_t k = 0; k < starts.size(); k++) {
        EXPECT(ends[k] >= starts[k]);
        out.spans.push_back(Span{starts[k], ends[k] + 1u - starts[k]});
    }
    return out;
}

static void check_cover(const u32 *len, const std::vector<u32> &len_copy, u32 n, u32 L, const Bytes *text) {
    const Cover got = run_core(len, n, L), want = brute_cover_of_len(len_copy, L);
    EXPECT(got.cov == want.cov);
    EXPECT(got.spans == want.spans);
    u64 covered = 0;
    for (size_t k = 0; k < got.spans.size(); k++) {
        covered += got.spans[k].len;
        if (k) EXPECT(got.spans[k - 1].s + got.spans[k - 1].len < got.spans[k].s);      // at least one byte apart
    }
    EXPECT(covered == (u64)std::count(got.cov.begin(), got.cov.end(), 1));
    g_spans += got.spans.size();
    if (text) {                                     // the mask and the dedup are the cover and the text, byte by byte
        Bytes kept;
        for (u32 p = 0; p < n; p++)
            if (!got.cov[p]) kept.push_back((*text)[p]);
        EXPECT(kept.size() == n - covered);
    }
}

struct Esa {
    std::unique_ptr<u32[]> sa, lcp;
};
static Esa esa_of(const Bytes &text) {
    const std::vector<u32> sa = sort_suffixes(text);
    return Esa{block_of(sa), block_of(lcp_of(text, sa))};
}

static void check_text(const Bytes &text, u32 lf) {
    const u32 n = (u32)text.size(), N = n + 1;
    const Esa e = esa_of(text);
    const MinTree lcp_tree = min_tree_of(e.lcp.get(), N, lf), sa_tree = min_tree_of(e.sa.get(), N, lf);
    const u32 nlev = lcp_tree.nlev;
    const u32 *lcp_min = lcp_tree.lmin.get(), *sa_min = sa_tree.lmin.get();
    memset(lz_climbed, 0, sizeof lz_climbed);
    memset(fm_ms_climbed, 0, sizeof fm_ms_climbed);
    const u32 params[][2] = {{1, 2}, {1, 4}, {2, 2}, {2, 3}, {3, 2}, {3, 3}, {5, 5}, {20, 2}, {n, 2}, {n + 1, 2}, {n > 1 ? n - 1 : 1, 2}, {1, n + 2}};
    for (const auto &pq : params) {
        const u32 L = pq[0], q = pq[1];
        if (L == 0) continue;
        for (int later = 0; later < 2; later++) {
            auto len = block<u32>(n);
            for (u32 i = 0; i < n; i++) len[i] = 0;
            const u64 by_rows = cov_seen[4];
            if (later) {
                launch(N, [&] { cov_seed_kernel<true>(e.sa.get(), e.lcp.get(), sa_min, lcp_min, N, lf, L, q, len.get()); });
            } else if (q == 2) {    // (the library builds no tree for this call)
                launch(N, [&] { cov_seed_kernel<false>(e.sa.get(), e.lcp.get(), nullptr, nullptr, N, lf, L, q, len.get()); });
            } else {
                launch(N, [&] { cov_seed_kernel<false>(e.sa.get(), e.lcp.get(), nullptr, lcp_min, N, lf, L, q, len.get()); });
            }
            const std::vector<u32> want = brute_seeds(text, L, q, later);
            std::vector<u32> got, copy(len.get(), len.get() + n);
            for (u32 i = 0; i < n; i++) {
                EXPECT(len[i] == 0 || len[i] == L);
                if (len[i]) got.push_back(i);
            }
            EXPECT(got == want);
            if (!later && q == 2) EXPECT(cov_seen[4] - by_rows == want.size());
            check_cover(len.get(), copy, n, L, &text);
            if (n <= 24 && L <= n) {
                const Cover c = brute_cover_of_len(copy, L);
                EXPECT(c.cov == brute_cover_by_substrings(text, L, q, later));
                for (const Span &s : c.spans) EXPECT(s.len >= L);
                EXPECT(c.spans.size() <= (n + 1) / (L + 1));
                g_counted++;
            }
            g_calls++;
            g_seeds += got.size();
        }
    }
    if (lf == 2) {
        for (u32 v = 0; v <= FM_MS_MAXLEV; v++) {
            g_down[v] += fm_ms_climbed[0][v];
            g_up[v] += fm_ms_climbed[1][v];
            g_min[v] += lz_climbed[v];
        }
        g_maxlev4 = std::max(g_maxlev4, nlev);
    }
    g_texts++;
}

// the general form over an array no text produces
static void check_array(const std::vector<u32> &v, u32 L) {
    const u32 n = (u32)v.size();
    auto len = block<u32>(n);
    std::copy(v.begin(), v.end(), len.get());
    check_cover(len.get(), v, n, L, nullptr);
    g_arrays++;
}

int main() {
    std::mt19937 rng(0xC0FE);
    for (u32 lf : {2u, 6u}) {
        for (u32 n : {1u, 2u, 3u, 5u, 8u, 13u, 17u, 24u, 40u, 63u, 64u, 65u, 257u, 300u, 640u, 1100u, 2200u}) {
            check_text(Bytes(n, 'A'), lf);
            for (u32 p : {2u, 3u, 7u}) check_text(periodic(n, p), lf);
            check_text(fibonacci(n), lf);
            for (u32 sigma : {1u, 2u, 4u, 200u}) check_text(random_text(rng, n, sigma), lf);
            if (n > 1100) continue;
            Bytes twice = random_text(rng, n, 4);   // a text followed by its own copy; a text whose last byte is new
            twice.insert(twice.end(), twice.begin(), twice.begin() + n);
            check_text(twice, lf);
            twice.back() = 'Z';
            check_text(twice, lf);
        }
        // one wide group that does not hold position 0: the range minimum over sa scans the top level of the fan-out-4 tree
        Bytes wide(2601, 'A');
        wide[0] = 'B';
        check_text(wide, lf);
    }
    // the general form
    const u32 T = COV_TILE;
    const u64 clamped = cov_seen[0], carried = g_carried;
    for (u32 n : {1u, 7u, 8u, 9u, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 4 * T + 100}) {
        check_array(std::vector<u32>(n, 0), 1);                         // nothing counts
        check_array(std::vector<u32>(n, 5), 5);                         // everything counts: one span (0, n)
        check_array(std::vector<u32>(n, 5), 6);                         // min_len above every entry
        check_array(std::vector<u32>(n, 0xffffffffu), 0xffffffffu);     // the 64-bit sum, the clamp
        std::vector<u32> v(n, 0);
        v[0] = 3 * T + 5;                                               // one entry and nothing else: tiles covered by the carry
        check_array(v, 1);
        v[0] = 0;
        v[n / 2] = 0xffffffffu;
        check_array(v, 2);
        for (u32 round = 0; round < 4; round++) {                       // random lengths, sparse and dense, short and long
            for (u32 &x : v) x = rng() % (round < 2 ? 50u : 3u) ? 0u : rng() % (round % 2 ? 3000u : 12u);
            for (u32 L : {1u, 2u, 7u, 2048u}) check_array(v, L);
        }
    }
    {
        std::vector<u32> v(3 * T, 0);
        v[5] = T - 5;                   // a reach that ends exactly on a tile boundary
        v[2 * T - 1] = 1;               // a span that starts on a tile's last position ...
        check_array(v, 1);
        v[2 * T - 1] = 0;
        v[T + 1] = T - 2;               // ... two spans one byte apart across a tile boundary: [T + 1, 2 T - 1) and [2 T, ...)
        v[2 * T] = 3;
        check_array(v, 1);
    }
    EXPECT(cov_seen[0] > clamped);                  // a reach clamped to n
    EXPECT(g_carried > carried);                    // a reach carried over a tile with no position that counts
    for (u32 v = 0; v <= g_maxlev4; v++) EXPECT(g_down[v] > 0 && g_up[v] > 0 && g_min[v] > 0);     // every level of the fan-out-4 tree
    EXPECT(g_maxlev4 >= 5);
    EXPECT(cov_seen[1] > 0 && cov_seen[2] > 0);     // a group of exactly q and of q - 1 rows
    EXPECT(cov_seen[3] > 0);                        // a leftmost occurrence refused under LATER
    EXPECT(cov_seen[4] > 0 && g_counted > 0);
    std::printf("ok: the repeat cover of %llu texts in %llu calls, %llu seeds, %llu spans, %llu arrays of the general form, %llu calls held "
                "against every substring; every tree level reached at fan-out 4 (%u levels) by both searches and by the range minimum\n",
                (unsigned long long)g_texts, (unsigned long long)g_calls, (unsigned long long)g_seeds, (unsigned long long)g_spans,
                (unsigned long long)g_arrays, (unsigned long long)g_counted, g_maxlev4);
    return 0;
}
