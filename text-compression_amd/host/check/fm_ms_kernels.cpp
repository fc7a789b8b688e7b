// Stand-alone host check of the matching-statistics kernels (csrc/tc_fm_ms.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/fm_ms_kernels.cpp -o fm_ms_kernels && ./fm_ms_kernels
// TC_FM_MS_HOST_CHECK compiles the bodies of the kernels as plain C++: the HIP keywords defined away, a workgroup of one
// lane, the lanes of a grid run one after another.  Every index is built naively -- suffixes sorted directly, the
// rank lines written in the 448-bit line format bit by bit, the LCP array by comparing neighbours, the min tree by
// fm_lmin_kernel level over level at fan-outs 4 and 64 -- in heap blocks of exactly the size the library allocates, so a
// read one element outside any of them stops the run.  What it walks:
//   - the two row searches alone, on arrays no text has (all large, sparse small values, random), against a linear scan,
//     from every row: this is where every level of the fan-out-4 tree is reached, in both directions;
//   - fm_ms_kernel, one lane per pattern, against brute force (substring search, the first row among directly sorted
//     suffixes, overlapping occurrences counted) on random texts of 1, 2, 4, 5 and 96 byte values with n on both sides of
//     a rank line and of a tree group, and on the texts whose shrinks cross many groups: unary, period 3, a Fibonacci
//     word, random binary, two letters with a rare third at the end; patterns: substrings, joined substrings, planted
//     substitutions, foreign bytes at either end and inside, empty, the whole text and twice over, random strings,
//     rare + short frequent string;
//   - the MEM kernels against the enumeration of all (i, l) that occur and are not contained in another.
// It asserts that no pattern took more than 2 m + 1 turns of the inner loop, and that both searches climbed to every
// level of a fan-out-4 tree at least once.

#define TC_FM_MS_HOST_CHECK
#include "tc_fm_ms.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

// ---- the min tree over an LCP array, by the library's kernel -------------------------------------------------------------
struct Tree {
    u32 N = 0, lf = 0;
    std::unique_ptr<u32[]> lcp;
    MinTree min;
    FmMsTree view() const { return min.view(lcp.get()); }
};
static void build_tree(Tree &t, const std::vector<u32> &lcp, u32 lf) {
    t.N = (u32)lcp.size();
    t.lf = lf;
    t.lcp = block_of(lcp);
    t.min = min_tree_of(t.lcp.get(), t.N, lf);
    EXPECT(t.min.nlev >= 1 && t.min.cnt[t.min.nlev] <= (1u << lf) && t.min.cnt[0] == t.N);
    for (u32 k = 1; k <= t.min.nlev; k++) {
        const u32 *dst = t.min.lmin.get() + t.min.off[k];
        for (u32 j = 0; j < t.min.cnt[k]; j++) {    // every entry is the minimum of the rows below it
            const u64 span = 1ull << (lf * k);
            u32 m = 0xffffffffu;
            for (u64 r = j * span; r < (j + 1) * span && r < t.N; r++) m = std::min(m, lcp[r]);
            EXPECT(dst[j] == m);
        }
    }
}

// ---- 1: the searches alone -------------------------------------------------------------------------------------------
static void check_searches(const std::vector<u32> &lcp, u32 lf, const std::vector<u32> &ds) {
    Tree t;
    build_tree(t, lcp, lf);
    const FmMsTree T = t.view();
    for (u32 d : ds)
        for (u32 r = 0; r < t.N; r++) {
            u32 want = r;
            while (lcp[want] >= d) want--;          // lcp[0] = 0 < d
            EXPECT(fm_ms_prev_below(T, r, d) == want);
            u32 up = r + 1;
            while (up < t.N && lcp[up] >= d) up++;
            EXPECT(fm_ms_next_below(T, t.N, r, d) == up);
        }
}
static void searches(std::mt19937 &rng) {
    for (u32 lf : {2u, 3u, 4u, 6u})
        for (u32 N : {1u, 2u, 3u, 4u, 5u, 63u, 64u, 65u, 255u, 256u, 257u, 1023u, 1101u, 1601u, 4097u, 4162u}) {
            std::vector<u32> a(N, 9);               // all large: the downward search ends at row 0, the upward one at N
            a[0] = 0;
            check_searches(a, lf, {1, 9, 10});
            std::vector<u32> b(N);                  // random small values
            for (u32 &v : b) v = rng() % 4;
            b[0] = 0;
            check_searches(b, lf, {1, 2, 3});
            std::vector<u32> c(N, 7);               // a few small values far apart
            c[0] = 0;
            for (int k = 0; k < 3; k++) c[rng() % N] = rng() % 7;
            c[0] = 0;
            check_searches(c, lf, {1, 4, 7});
        }
}

// ---- 2: an index, naively ----------------------------------------------------------------------------------------------
struct Index {
    Bytes text;
    u32 n = 0, N = 0, sigma = 0;
    u64 lines = 0;
    std::vector<u32> sa, rank, lcp;
    std::unique_ptr<u64[]> bits;
    std::unique_ptr<u32[]> tab, sa_blk;
    Tree tree;
};
static void build_index(Index &ix, const Bytes &text, u32 lf) {
    ix.text = text;
    const u32 n = ix.n = (u32)text.size(), N = ix.N = n + 1;
    ix.sa = sort_suffixes(text);
    ix.rank = inverse_of(ix.sa);
    ix.lcp = lcp_of(text, ix.sa);
    u32 counts[256] = {};
    for (u8 b : text) counts[b]++;
    ix.tab = block<u32>(768);                       // fm_make_tab of csrc/tc_fm_host.hpp
    u32 sig = 0, acc = 1;
    for (int b = 0; b < 256; b++) {
        ix.tab[b] = 0xFFFFFFFFu;
        if (counts[b]) {
            ix.tab[b] = sig;
            ix.tab[256 + sig] = acc;
            ix.tab[512 + sig] = counts[b];
            acc += counts[b];
            sig++;
        }
    }
    for (u32 c = sig; c < 256; c++) ix.tab[256 + c] = ix.tab[512 + c] = 0;
    ix.sigma = sig;
    ix.lines = N / FM_LINE_BITS + 1;
    ix.bits = block<u64>((size_t)sig * ix.lines * 8);
    std::memset(ix.bits.get(), 0, (size_t)sig * ix.lines * 64);
    std::vector<u64> ones(sig, 0);
    for (u32 j = 0; j < N; j++) {                   // bit j of vector c: L[j] = c, the primary row (sa = 0) in none
        const u64 line = j / FM_LINE_BITS;
        const u32 off = j % FM_LINE_BITS;
        if (off == 0)
            for (u32 c = 0; c < sig; c++) ix.bits[((u64)c * ix.lines + line) * 8] = ones[c];
        if (ix.sa[j] == 0) continue;
        const u32 c = ix.tab[text[ix.sa[j] - 1]];
        ix.bits[((u64)c * ix.lines + line) * 8 + 1 + off / 64] |= 1ull << (off % 64);
        ones[c]++;
    }
    if (N % FM_LINE_BITS == 0)                      // the line behind the last row exists and carries the totals
        for (u32 c = 0; c < sig; c++) ix.bits[((u64)c * ix.lines + ix.lines - 1) * 8] = ones[c];
    ix.sa_blk = block<u32>(N);
    std::memcpy(ix.sa_blk.get(), ix.sa.data(), (size_t)N * 4);
    build_tree(ix.tree, ix.lcp, lf);
}

// brute force of one pattern: ms_len by comparing with every text position, the first row and the width from them
static void brute(const Index &ix, const Bytes &p, std::vector<u32> &len, std::vector<u64> &pos, std::vector<u32> &occ) {
    const u32 m = (u32)p.size(), n = ix.n;
    len.assign(m, 0); pos.assign(m, 0); occ.assign(m, 0);
    std::vector<u32> cp(n + 1);
    for (u32 i = 0; i < m; i++) {
        u32 best = 0;
        for (u32 t = 0; t < n; t++) {
            u32 l = 0;
            while (i + l < m && t + l < n && p[i + l] == ix.text[t + l]) l++;
            cp[t] = l;
            best = std::max(best, l);
        }
        if (!best) continue;
        u32 first = 0xffffffffu, k = 0;
        for (u32 t = 0; t < n; t++)
            if (cp[t] >= best) {
                k++;
                first = std::min(first, ix.rank[t]);
            }
        len[i] = best;
        pos[i] = (u64)ix.sa[first] + 1;
        occ[i] = k;
    }
}

// MEMs by enumeration: all (i, l) with p[i .. i + l) in the text -- exactly the l <= ms_len[i] -- that are contained in
// no other such pair; a pair (i2, l2) that contains (i, l) exists exactly when the longest one at i2 does
static void brute_mems(const std::vector<u32> &len, std::vector<u64> &starts, std::vector<u32> &lens) {
    const u32 m = (u32)len.size();
    starts.clear();
    lens.clear();
    for (u32 i = 0; i < m; i++)
        for (u32 l = 1; l <= len[i]; l++) {
            bool inside = l < len[i];
            for (u32 i2 = 0; i2 < i && !inside; i2++) inside = i2 + len[i2] >= i + l;
            if (!inside) {
                starts.push_back(i);
                lens.push_back(l);
            }
        }
}

static u64 g_patterns = 0, g_positions = 0, g_worst_turns_num = 0, g_worst_turns_m = 1;

static void check_batch(const Index &ix, const std::vector<Bytes> &pats, bool sampled) {
    const u64 npat = pats.size();
    std::vector<u64> offs(npat + 1, 0);
    for (u64 i = 0; i < npat; i++) offs[i + 1] = offs[i] + pats[i].size();
    const u64 total = offs[npat];
    // the pattern bytes between two aligned words of slack: the kernel's 4-byte window reads the aligned word around a byte
    auto flat = block<u8>(total + 8);
    u8 *fp = flat.get() + 4;
    for (u64 i = 0; i < npat; i++)
        if (!pats[i].empty()) std::memcpy(fp + offs[i], pats[i].data(), pats[i].size());
    auto d_offs = block<u64>(npat + 1);
    std::memcpy(d_offs.get(), offs.data(), (npat + 1) * 8);
    auto ms_len = block<u32>(total), ms_occ = block<u32>(total), ms_len0 = block<u32>(total);
    auto ms_pos = block<u64>(total);
    const u32 *sa = sampled ? nullptr : ix.sa_blk.get();
    for (fm_ms_block = 0; fm_ms_block < npat; fm_ms_block++) {
        fm_ms_turns = 0;
        fm_ms_kernel<true>(ix.bits.get(), ix.lines, ix.tab.get(), ix.N, ix.tree.lcp.get(), ix.tree.min.lmin.get(), ix.tree.lf, sa, fp,
                           d_offs.get(), npat, ms_len.get(), ms_pos.get(), ms_occ.get());
        const u64 m = pats[fm_ms_block].size();
        EXPECT(fm_ms_turns <= 2 * m + 1);
        if (m && fm_ms_turns * g_worst_turns_m > g_worst_turns_num * m) g_worst_turns_num = fm_ms_turns, g_worst_turns_m = m;
    }
    launch(npat, [&] {
        fm_ms_kernel<false>(ix.bits.get(), ix.lines, ix.tab.get(), ix.N, ix.tree.lcp.get(), ix.tree.min.lmin.get(), ix.tree.lf, sa, fp,
                            d_offs.get(), npat, ms_len0.get(), nullptr, nullptr);
    });
    std::vector<u32> len, occ;
    std::vector<u64> pos, mems;
    std::vector<u32> mem_lens;
    for (u64 p = 0; p < npat; p++) {
        brute(ix, pats[p], len, pos, occ);
        for (u64 i = 0; i < pats[p].size(); i++) {
            const u64 o = offs[p] + i;
            EXPECT(ms_len[o] == len[i] && ms_len0[o] == len[i] && ms_occ[o] == occ[i]);
            if (sampled) EXPECT(ms_pos[o] == (len[i] ? (u64)ix.rank[pos[i] - 1] : 0));     // the row itself
            else EXPECT(ms_pos[o] == pos[i]);
        }
        g_patterns++;
        g_positions += pats[p].size();
    }
    // the MEM kernels over these statistics
    for (u32 min_len : {1u, 2u, 5u, 20u}) {
        auto cnt = block<i64>(npat);
        launch(npat, [&] { fm_mem_count_kernel(ms_len.get(), d_offs.get(), npat, min_len, cnt.get()); });
        auto moffs = block<u64>(npat + 1);
        moffs[0] = 0;
        for (u64 p = 0; p < npat; p++) moffs[p + 1] = moffs[p] + (u64)cnt[p];
        const u64 nm = moffs[npat];
        auto mstart = block<u64>(nm), mpos = block<u64>(nm);
        auto mlen = block<u32>(nm);
        launch(npat, [&] {
            fm_mem_fill_kernel(ms_len.get(), ms_pos.get(), d_offs.get(), npat, min_len, moffs.get(), mstart.get(), mpos.get(),
                               mlen.get());
        });
        for (u64 p = 0; p < npat; p++) {
            std::vector<u32> l(ms_len.get() + offs[p], ms_len.get() + offs[p + 1]);
            brute_mems(l, mems, mem_lens);
            u64 k = 0;
            for (u64 x = 0; x < mems.size(); x++) {
                if (mem_lens[x] < min_len) continue;
                const u64 o = moffs[p] + k++, i = mems[x];
                EXPECT(k <= (u64)cnt[p]);
                EXPECT(mstart[o] == i && mlen[o] == mem_lens[x] && mlen[o] == l[i] && mpos[o] == ms_pos[offs[p] + i]);
            }
            EXPECT(k == (u64)cnt[p]);
        }
    }
}

// ---- texts and patterns ------------------------------------------------------------------------------------------------
static Bytes sub(std::mt19937 &rng, const Bytes &t, u32 m) {
    m = std::min<u32>(m, (u32)t.size());
    const u32 o = rng() % (t.size() - m + 1);
    return Bytes(t.begin() + o, t.begin() + o + m);
}
static Bytes cat(const Bytes &a, const Bytes &b) {
    Bytes r(a);
    r.insert(r.end(), b.begin(), b.end());
    return r;
}
static std::vector<Bytes> patterns(std::mt19937 &rng, const Bytes &t, const Bytes &al, const Bytes &foreign) {
    std::vector<Bytes> P;
    for (u32 m : {1u, 2u, 3u, 17u, 100u}) P.push_back(sub(rng, t, m));
    P.push_back(cat(sub(rng, t, 40), sub(rng, t, 40)));
    P.push_back(cat(cat(sub(rng, t, 17), sub(rng, t, 1)), sub(rng, t, 17)));
    for (u32 planted : {1u, 2u, 4u}) {
        Bytes p = sub(rng, t, 60);
        for (u32 k = 0; k < planted; k++) p[rng() % p.size()] = al[rng() % al.size()];
        P.push_back(p);
    }
    if (!foreign.empty()) {
        const Bytes f1(1, foreign[0]), f2(1, foreign.back()), mid = sub(rng, t, 17);
        P.push_back(cat(f1, mid));
        P.push_back(cat(mid, f2));
        P.push_back(cat(cat(mid, f1), mid));
        P.push_back(foreign);
    }
    P.push_back(Bytes());
    if (t.size() <= 150) {
        P.push_back(t);
        P.push_back(cat(t, t));
    }
    for (u32 m : {1u, 2u, 5u, 33u}) P.push_back(random_text(rng, m, al));
    return P;
}

int main() {
    std::mt19937 rng(0x5f01);
    searches(rng);
    for (int dir = 0; dir < 2; dir++) {
        // N = 1601 at fan-out 4: 401, 101, 26, 7 and 2 entries -- five tree levels, every one of them scanned
        u32 off[FM_MS_MAXLEV + 1], cnt[FM_MS_MAXLEV + 1], words;
        const u32 nlev = fm_ms_tree_shape(1601, 2, off, cnt, &words);
        EXPECT(nlev == 5);
        for (u32 l = 0; l <= nlev; l++) EXPECT(fm_ms_climbed[dir][l] > 0);
    }
    const Bytes foreign = {0, 7, 255};
    const std::vector<Bytes> alphabets = {{'A'}, {'A', 'C'}, {'A', 'C', 'G', 'T'}, {'A', 'C', 'G', 'N', 'T'}};
    for (u32 lf : {2u, 6u}) {
        for (u32 n : {1u, 2u, 63u, 64u, 65u, 447u, 448u, 449u, 897u})
            for (const Bytes &al : alphabets) {
                if (n > 449 && al.size() == 2) continue;
                Index ix;
                build_index(ix, random_text(rng, n, al), lf);
                check_batch(ix, patterns(rng, ix.text, al, foreign), n % 2 == 0);
            }
        {
            Bytes al96;
            for (int b = 32; b < 128; b++) al96.push_back((u8)b);
            Index ix;
            build_index(ix, random_text(rng, 700, al96), lf);
            check_batch(ix, patterns(rng, ix.text, al96, foreign), false);
        }
        // shrinks that cross many groups
        const u32 n = lf == 2 ? 1100 : 1300;
        std::vector<std::pair<Bytes, Bytes>> shapes;
        shapes.push_back({Bytes(n, 'A'), Bytes{'A'}});
        shapes.push_back({periodic(n, 3), Bytes{'A', 'C', 'G'}});
        shapes.push_back({fibonacci(n), Bytes{'A', 'B'}});
        shapes.push_back({random_text(rng, n, Bytes{'A', 'B'}), Bytes{'A', 'B'}});
        for (auto &sh : shapes) {
            Index ix;
            build_index(ix, sh.first, lf);
            std::vector<Bytes> P = patterns(rng, ix.text, sh.second, foreign);
            P.push_back(cat(Bytes(200, sh.second[0]), Bytes(1, sh.second.back())));
            P.push_back(cat(sub(rng, ix.text, 150), cat(Bytes(1, sh.second[0]), sub(rng, ix.text, 150))));
            check_batch(ix, P, false);
        }
        {
            Bytes t = random_text(rng, n - 1, Bytes{'A', 'B'});
            t.push_back('Z');                       // one rare letter, only at the end
            Index ix;
            build_index(ix, t, lf);
            std::vector<Bytes> P = patterns(rng, ix.text, Bytes{'A', 'B'}, foreign);
            for (const char *tail : {"A", "B", "AA", "AB", "BA", "BB", "ABA", "BBB", "BAB"}) {
                const Bytes w(tail, tail + std::strlen(tail));
                P.push_back(cat(Bytes{'Z'}, w));    // fails at depth 1 .. 3 on intervals of hundreds of rows
                P.push_back(cat(cat(w, Bytes{'Z'}), w));
            }
            check_batch(ix, P, true);
        }
    }
    std::printf("ok: matching statistics of %llu patterns, %llu positions; most turns per byte %.3f (bound 2 + 1/m)\n",
                (unsigned long long)g_patterns, (unsigned long long)g_positions, (double)g_worst_turns_num / (double)g_worst_turns_m);
    return 0;
}
