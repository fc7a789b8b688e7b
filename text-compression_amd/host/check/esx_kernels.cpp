// Stand-alone host check of the cross-document matches on the kept enhanced suffix array (csrc/tc_esa_xdoc.hpp), meant to be built
// with a host sanitizer:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/esx_kernels.cpp -o esx_kernels && ./esx_kernels
// TC_FM_MS_HOST_CHECK compiles both instances of esx_match_kernel, with the row searches of csrc/tc_fm_ms.hpp and the range minimum
// of csrc/tc_lz.hpp, and the lane bodies of the scans and of the per-document sums as plain C++, as host/check/esa_docs_kernels.cpp
// does for the document queries: the HIP keywords defined away, the lanes run one after another.  What the device does across the
// lanes of a workgroup and across tiles -- the scans -- is a plain loop over the lanes' values here.  Everything around the lanes
// is built naively -- suffixes sorted directly, lcp by comparing neighbours, da by a loop, the min trees of lcp and da by
// fm_lmin_kernel at fan-outs 4 and 64 -- in heap blocks of exactly the entries the library allocates, so a read or a store one
// element outside any of them stops the run.  Every answer is compared with loops over the bytes.  The program asserts what no
// device test sees: every level of a five-level tree reached by both da searches and by the range minima, the "no qualifying row"
// outcome on each side and on both, a run longer than two tiles, a run head in an earlier tile, the clamp fired, empty documents
// first, last and adjacent, and a da and trees of arbitrary contents that keep every access in bounds.

#define TC_FM_MS_HOST_CHECK
#include "tc_esa_xdoc.hpp"
#include "check_esa.hpp"      // launch, MinTree; EXPECT, the blocks, the naive suffix array and the texts (check_common.hpp)

static u64 g_texts = 0, g_rows = 0, g_garbage = 0;
static bool g_long_run = false, g_far_head = false, g_empty_first = false, g_empty_last = false, g_empty_adjacent = false;
static u64 g_da_up[2][FM_MS_MAXLEV + 1] = {}, g_rmq_up[FM_MS_MAXLEV + 1] = {};

// ---- the handle, naively, in exact sizes
struct Esa {
    u32 n, N, lf, nlev, words, ndocs;
    std::vector<u32> ds;
    std::unique_ptr<u32[]> doc_start, sa, lcp, da, lcp_min, da_min;
};
static u32 doc_of(const std::vector<u32> &ds, u32 p) {
    for (u32 d = 0; d + 1 < ds.size(); d++)
        if (ds[d] <= p && p < ds[d + 1]) return d;
    return ESD_NO_DOC;
}
static Esa esa_of(const Bytes &t, const std::vector<u32> &ds, u32 lf) {
    Esa e;
    e.n = (u32)t.size();
    e.N = e.n + 1;
    e.lf = lf;
    e.ds = ds;
    e.ndocs = (u32)ds.size() - 1;
    const u32 N = e.N;
    e.doc_start = block<u32>(ds.size(), 0);
    std::copy(ds.begin(), ds.end(), e.doc_start.get());
    // (the library rounds a row array up to 16 bytes: the 16-byte loads of the searches stay inside; fm_ms_load4 masks here)
    const std::vector<u32> sa = sort_suffixes(t);
    e.sa = block_of(sa);
    e.lcp = block_of(lcp_of(t, sa));
    e.da = block<u32>(N, 0);
    for (u32 j = 0; j < N; j++) e.da[j] = doc_of(ds, e.sa[j]);
    MinTree lcp_tree = min_tree_of(e.lcp.get(), N, lf), da_tree = min_tree_of(e.da.get(), N, lf);
    e.nlev = lcp_tree.nlev;
    e.words = lcp_tree.words;
    e.lcp_min = std::move(lcp_tree.lmin);
    e.da_min = std::move(da_tree.lmin);
    return e;
}

// ---- brute force over the bytes
struct Want { std::vector<u32> xl, src, xdoc; };
static Want brute(const Bytes &t, const Esa &e, int kind, bool clamp, u32 *none_a, u32 *none_b) {
    const u32 n = e.n, N = e.N;
    Want w;
    w.xl.assign(n, 0); w.src.assign(n, ESX_NO_POS); w.xdoc.assign(n, ESD_NO_DOC);
    for (u32 r = 1; r < N; r++) {
        const u32 i = e.sa[r], d = e.da[r];
        long best = -1;
        u32 partner = 0;
        for (int step = -1; step <= 1; step += 2) {         // the predecessor first: it wins a tie
            long x = (long)r + step;
            while (x >= 1 && x < (long)N && !(kind == ESX_OTHER ? e.da[x] != d : e.da[x] < d)) x += step;
            if (x < 1 || x >= (long)N) {
                (step < 0 ? *none_a : *none_b)++;
                continue;
            }
            const u32 j = e.sa[x];
            long l = 0;
            while (i + l < n && j + l < n && t[i + l] == t[j + l]) l++;
            if (l > best) { best = l; partner = j; }
        }
        if (best > 0) {
            w.xl[i] = (u32)best; w.src[i] = partner; w.xdoc[i] = doc_of(e.ds, partner);
            if (clamp) w.xl[i] = std::min<u32>((u32)best, e.ds[d + 1] - i);
        }
    }
    return w;
}

// ---- the run heads: esx_bmask and esx_lane_heads lane after lane, the scans of the workgroup and of the tiles as loops
static void heads(const u32 *da, u32 N, u32 *up, u32 *dn) {
    const u64 lanes = ((u64)N + ESX_ROWS - 1) / ESX_ROWS;
    std::vector<u32> mask(lanes), last1(lanes), first(lanes);
    for (u64 j = 0; j < lanes; j++) {
        const u64 base = j * ESX_ROWS;
        u32 w[ESX_ROWS + 1];
        for (u32 k = 0; k <= ESX_ROWS; k++) {               // (esx_load_da)
            const u64 r1 = base + k;
            w[k] = r1 >= 1 && r1 <= N ? da[r1 - 1] : 0u;
        }
        mask[j] = esx_bmask(w, base, N);
        last1[j] = esx_last1(mask[j], base);
        first[j] = esx_first(mask[j], base, N);
    }
    std::vector<u32> prev1(lanes), next(lanes);
    u32 run = 0;
    for (u64 j = 0; j < lanes; j++) { prev1[j] = run; run = std::max(run, last1[j]); }
    run = N;
    for (u64 j = lanes; j-- > 0;) { next[j] = run; run = std::min(run, first[j]); }
    for (u64 j = 0; j < lanes; j++) {
        esx_lane_heads(mask[j], j * ESX_ROWS, N, prev1[j], next[j], up, dn);
        // a head in an earlier tile: the lane's rows start with a run whose head lies before the lane's tile
        if (prev1[j] && (prev1[j] - 1) / ESX_TILE < (j * ESX_ROWS) / ESX_TILE && !(mask[j] & 1u)) g_far_head = true;
    }
}

// ---- the per-document answers from the clamped lengths, through the lane bodies
static void doc_answers(const Esa &e, const std::vector<u32> &xl, u32 min_len, std::vector<u64> &shared, std::vector<u32> &longest) {
    const u32 n = e.n, nd = e.ndocs;
    const u32 *ds = e.doc_start.get();
    // the cover, as cov_mask_kernel leaves it: one byte per position, exactly n bytes
    auto cov = block<u8>(n, 0);
    u64 reach = 0;
    for (u32 i = 0; i < n; i++) {
        if (xl[i] >= min_len) reach = std::max<u64>(reach, std::min<u64>(n, (u64)i + xl[i]));
        cov[i] = reach > i;
    }
    const u64 stiles = ((u64)n + ESX_STILE - 1) / ESX_STILE + 1;
    std::vector<u64> tbase(stiles, 0);
    u64 acc = 0;
    for (u64 t = 0; t < stiles; t++) {
        tbase[t] = acc;
        for (u32 l = 0; l < ESX_NT; l++) acc += esx_lane_sum(cov.get(), t * ESX_STILE + (u64)l * ESX_SBYTES, n);
    }
    std::vector<u64> pre(nd + 1);
    for (u32 j = 0; j <= nd; j++) {                          // (esx_doc_prefix_kernel)
        const u64 p = ds[j], t = p / ESX_STILE;
        EXPECT(t < stiles);
        u64 s = 0;
        for (u32 l = 0; l < ESX_NT; l++) s += esx_lane_sum(cov.get(), t * ESX_STILE + (u64)l * ESX_SBYTES, p);
        pre[j] = tbase[t] + s;
    }
    shared.assign(nd, 0);
    for (u32 d = 0; d < nd; d++) shared[d] = pre[d + 1] - pre[d];
    // the segmented maximum (esx_seg_kernel): per tile the start bits, the lanes' values joined in order, the documents that end here
    auto len = block<u32>(n, 0);
    std::copy(xl.begin(), xl.end(), len.get());
    auto out = block<u32>(nd, 0);
    const u64 ptiles = ((u64)n + ESX_TILE - 1) / ESX_TILE;
    u64 carry = 0;
    for (u64 t = 0; t < ptiles; t++) {
        const u64 tb = t * ESX_TILE, te = tb + ESX_TILE;
        u32 bits[ESX_TILE / 32] = {};
        for (u32 d = esx_lower(ds, nd, tb); d < nd; d++) {
            const u64 s = ds[d];
            if (s >= te) break;
            if (s >= tb) bits[(u32)(s - tb) >> 5] |= 1u << ((u32)(s - tb) & 31u);
        }
        u32 m[ESX_TILE];
        u64 run = carry, tile = 0;
        for (u32 l = 0; l < ESX_NT; l++) {
            const u64 base = tb + (u64)l * ESX_ROWS;
            u32 v[ESX_ROWS];
            for (u32 k = 0; k < ESX_ROWS; k++) v[k] = base + k < n ? len[base + k] : 0u;
            const u32 starts = (bits[l >> 2] >> ((l & 3u) * ESX_ROWS)) & ((1u << ESX_ROWS) - 1u);
            tile = esx_seg_join(tile, esx_seg_lane(0, v, starts, nullptr));
            run = esx_seg_lane(run, v, starts, m + l * ESX_ROWS);
        }
        EXPECT((u32)run == (u32)esx_seg_join(carry, tile));      // what the two passes of the device compute is one value
        carry = esx_seg_join(carry, tile);
        for (u32 j = esx_lower(ds, nd, tb + 1u); j <= nd; j++) {
            const u64 en = ds[j];
            if (en > te || j == 0) break;
            const u64 s = ds[j - 1u];
            EXPECT(en > tb && en - 1u - tb < ESX_TILE);
            out[j - 1u] = s < en ? m[(u32)(en - 1u - tb)] : 0u;
        }
    }
    longest.assign(out.get(), out.get() + nd);
}

static void check_collection(const Bytes &t, const std::vector<u32> &ds, u32 lf, u32 none[2][3]) {
    const Esa e = esa_of(t, ds, lf);
    const u32 n = e.n, N = e.N;
    if (n == 0) return;
    auto up = block<u32>(N, 0xabababab), dn = block<u32>(N, 0xabababab);
    heads(e.da.get(), N, up.get(), dn.get());
    for (u32 r = 1, head = 1; r < N; r++) {                  // against a walk over the rows
        if (e.da[r] != e.da[r - 1]) head = r;
        u32 nx = r + 1;
        while (nx < N && e.da[nx] == e.da[nx - 1]) nx++;
        EXPECT(up[r] == head - 1 && dn[r] == nx);
        if (r - head > 2 * ESX_TILE) g_long_run = true;
    }
    for (int kind = 0; kind < 2; kind++) {
        Want clamped;
        for (int clamp = 0; clamp < 2; clamp++) {
            u32 na = 0, nb = 0;
            const Want w = brute(t, e, kind, clamp != 0, &na, &nb);
            for (u32 outs : {1u, 6u, 7u}) {                            // xl alone, src and xdoc alone, all three
                auto xl = block<u32>(n, 0xabababab), src = block<u32>(n, 0xabababab), xdoc = block<u32>(n, 0xabababab);
                const u64 seen0 = esx_seen[0], seen1 = esx_seen[1], seen2 = esx_seen[2];
                memset(fm_ms_climbed, 0, sizeof fm_ms_climbed);
                memset(lz_climbed, 0, sizeof lz_climbed);
                launch(n, [&] {
                    if (kind == ESX_OTHER)
                        esx_match_kernel<ESX_OTHER>(n, e.sa.get(), e.lcp.get(), e.lcp_min.get(), e.da.get(), nullptr, up.get(), dn.get(),
                                                    e.doc_start.get(), e.ndocs, lf, (u32)clamp, outs & 1 ? xl.get() : nullptr,
                                                    outs & 2 ? src.get() : nullptr, outs & 4 ? xdoc.get() : nullptr);
                    else
                        esx_match_kernel<ESX_EARLIER>(n, e.sa.get(), e.lcp.get(), e.lcp_min.get(), e.da.get(), e.da_min.get(), nullptr, nullptr,
                                                      e.doc_start.get(), e.ndocs, lf, (u32)clamp, outs & 1 ? xl.get() : nullptr,
                                                      outs & 2 ? src.get() : nullptr, outs & 4 ? xdoc.get() : nullptr);
                });
                if (lf == 2 && e.nlev == 4) {
                    for (u32 k = 0; k <= FM_MS_MAXLEV; k++) {
                        g_da_up[0][k] += fm_ms_climbed[0][k];
                        g_da_up[1][k] += fm_ms_climbed[1][k];
                        g_rmq_up[k] += lz_climbed[k];
                    }
                }
                for (u32 i = 0; i < n; i++) {
                    EXPECT(xl[i] == (outs & 1 ? w.xl[i] : 0xabababab));
                    EXPECT(src[i] == (outs & 2 ? w.src[i] : 0xabababab));
                    EXPECT(xdoc[i] == (outs & 4 ? w.xdoc[i] : 0xabababab));
                }
                // the outcomes the kernel counted are the ones the walk met
                const u64 k0 = esx_seen[0] - seen0, k1 = esx_seen[1] - seen1, k2 = esx_seen[2] - seen2;
                EXPECT(k0 + k2 == na && k1 + k2 == nb);
                none[kind][0] += (u32)k0; none[kind][1] += (u32)k1; none[kind][2] += (u32)k2;
                g_rows += n;
            }
            if (clamp) clamped = w;
        }
        for (u32 min_len : {1u, 2u, 3u, 20u}) {
            std::vector<u64> shared;
            std::vector<u32> longest;
            doc_answers(e, clamped.xl, min_len, shared, longest);
            for (u32 d = 0; d < e.ndocs; d++) {
                u64 s = 0;
                u32 m = 0;
                for (u32 p = ds[d]; p < ds[d + 1]; p++) {
                    bool c = false;
                    for (u32 i = ds[d]; i <= p && !c; i++) c = clamped.xl[i] >= min_len && p < i + clamped.xl[i];
                    s += c;
                    m = std::max(m, clamped.xl[p]);
                }
                EXPECT(shared[d] == s && longest[d] == m);
            }
        }
    }
    if (e.ndocs >= 2) {
        g_empty_first |= ds[1] == 0;
        g_empty_last |= ds[e.ndocs - 1] == n;
        for (u32 d = 1; d + 1 < e.ndocs; d++) g_empty_adjacent |= ds[d] == ds[d + 1] && ds[d - 1] == ds[d] && ds[d] > 0 && ds[d] < n;
    }
    g_texts++;
}

// a da, an up / dn and trees of arbitrary contents: nothing is compared, every access must stay inside the blocks
static void check_garbage(u32 n, u32 lf, std::mt19937 &rng) {
    Bytes t(n);
    for (auto &c : t) c = (u8)('a' + rng() % 2);
    std::vector<u32> ds = {0, n / 3, n};
    Esa e = esa_of(t, ds, lf);
    const u32 N = e.N;
    auto up = block<u32>(N, 0), dn = block<u32>(N, 0);
    for (u32 round = 0; round < 4; round++) {
        for (u32 r = 0; r < N; r++) {
            e.da[r] = round == 0 ? rng() : rng() % 4;
            up[r] = round < 2 ? rng() : rng() % (N + 2);
            dn[r] = round < 2 ? rng() : rng() % (N + 2);
        }
        for (u32 k = 0; k < e.words; k++) {
            e.da_min[k] = round % 2 ? rng() % 4 : rng();
            e.lcp_min[k] = rng() % 8;
        }
        auto xl = block<u32>(n, 0), src = block<u32>(n, 0), xdoc = block<u32>(n, 0);
        launch(n, [&] {
            esx_match_kernel<ESX_OTHER>(n, e.sa.get(), e.lcp.get(), e.lcp_min.get(), e.da.get(), nullptr, up.get(), dn.get(), e.doc_start.get(),
                                        e.ndocs, lf, 1u, xl.get(), src.get(), xdoc.get());
        });
        launch(n, [&] {
            esx_match_kernel<ESX_EARLIER>(n, e.sa.get(), e.lcp.get(), e.lcp_min.get(), e.da.get(), e.da_min.get(), nullptr, nullptr,
                                          e.doc_start.get(), e.ndocs, lf, 1u, xl.get(), src.get(), xdoc.get());
        });
        heads(e.da.get(), N, up.get(), dn.get());
        for (u32 r = 0; r < N; r++) EXPECT(up[r] < N && dn[r] <= N);
        g_garbage++;
    }
}

int main() {
    std::mt19937 rng(0xE5C);
    u32 none[2][3] = {};
    for (u32 lf : {2u, 6u}) {
        // every text over {a, b} up to 5 bytes with every split into at most 3 documents
        for (u32 n = 0; n <= 5; n++)
            for (u32 bits = 0; bits < (1u << n); bits++) {
                Bytes t(n);
                for (u32 i = 0; i < n; i++) t[i] = (u8)('a' + ((bits >> i) & 1u));
                check_collection(t, {0, n}, lf, none);
                for (u32 a = 0; a <= n; a++) {
                    check_collection(t, {0, a, n}, lf, none);
                    for (u32 b = a; b <= n; b++) check_collection(t, {0, a, b, n}, lf, none);
                }
            }
        std::vector<Bytes> texts;
        for (u32 n : {37u, 300u, 700u}) {
            Bytes r2(n), r4(n), per(n), un(n, 'a');
            for (u32 i = 0; i < n; i++) {
                r2[i] = (u8)('a' + rng() % 2);
                r4[i] = (u8)('a' + rng() % 4);
                per[i] = (u8)"abcabca"[i % 7];
            }
            texts.push_back(r2); texts.push_back(r4); texts.push_back(per); texts.push_back(un); texts.push_back(fibonacci(n, 'a', 'b'));
        }
        for (const Bytes &t : texts) {
            const u32 n = (u32)t.size();
            check_collection(t, {0, n}, lf, none);
            check_collection(t, {0, n / 2, n}, lf, none);
            check_collection(t, {0, 0, n / 5, n / 5, n / 5, n / 2, n, n}, lf, none);       // empty documents first, last and adjacent
            std::vector<u32> each(n + 1);
            for (u32 i = 0; i <= n; i++) each[i] = i;
            check_collection(t, each, lf, none);
            std::vector<u32> cut = {0};
            for (u32 i = 0; i < 12; i++) cut.push_back(rng() % (n + 1));
            cut.push_back(n);
            std::sort(cut.begin(), cut.end());
            check_collection(t, cut, lf, none);
        }
        // a one-byte document that sorts first / last: every other row searches across the whole tree for it
        for (u8 c : {(u8)'A', (u8)'z'}) {
            Bytes t(600);
            for (auto &x : t) x = (u8)('a' + rng() % 2);
            t[0] = c;
            check_collection(t, {0, 1, 600}, lf, none);
            t[0] = 'a';
            t[599] = c;
            check_collection(t, {0, 599, 600}, lf, none);
        }
        // the same on a unary text, where no lcp between the two rows is 0 and the range minimum climbs as far as the search
        {
            Bytes t(600, 'a');
            check_collection(t, {0, 1, 600}, lf, none);
            check_collection(t, {0, 599, 600}, lf, none);
        }
        // a run of one document over more than two tiles, heads in earlier tiles; documents that end in later tiles
        {
            Bytes t(2 * ESX_TILE + 600, 'a');
            t.push_back('b');
            t.push_back('a');
            const u32 n = (u32)t.size();
            check_collection(t, {0, n - 2, n}, lf, none);
            check_collection(t, {0, 5, ESX_TILE, ESX_TILE, ESX_TILE + 1, n}, lf, none);
        }
        for (u32 n : {1u, 9u, 257u, 1025u}) check_garbage(n, lf, rng);
    }
    for (int kind = 0; kind < 2; kind++)
        for (int k = 0; k < 3; k++) EXPECT(none[kind][k] > 0);              // no qualifying row above, below, on both sides
    for (u32 k = 0; k <= 4; k++) {
        EXPECT(g_da_up[0][k] > 0 && g_da_up[1][k] > 0);                     // both da searches climbed to every level of a five-level tree
        EXPECT(g_rmq_up[k] > 0);                                            // and so did the range minima
    }
    EXPECT(esx_seen[3] > 0 && esx_seen[4] > 0 && esx_seen[5] > 0 && esx_seen[6] > 0 && esx_seen[7] > 0);
    EXPECT(esx_seen[8] > 0 && esx_seen[9] > 0);                             // (the arbitrary arrays)
    EXPECT(g_long_run && g_far_head && g_empty_first && g_empty_last && g_empty_adjacent);
    std::printf("ok: the cross-document matches of %llu collections, %llu rows, %llu arbitrary arrays; every tree level reached at fan-out 4\n",
                (unsigned long long)g_texts, (unsigned long long)g_rows, (unsigned long long)g_garbage);
    return 0;
}
