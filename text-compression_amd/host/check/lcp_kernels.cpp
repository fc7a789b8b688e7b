// Stand-alone host check of the LCP kernels (csrc/tc_lcp.hpp), meant to be built with a host sanitizer:
//   g++ -O1 -g -std=c++17 -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/lcp_kernels.cpp -o lcp_kernels && ./lcp_kernels
// (-Wno-unknown-pragmas: csrc/tc_lcp.hpp carries a "#pragma unroll" the host compiler does not know.)
// TC_LCP_HOST_CHECK compiles the bodies of the kernels as plain C++: the HIP keywords defined away, a workgroup of one
// lane, the workgroups of a grid run one after another in the launch order of lcp_device (csrc/tc_lcp_host.hpp): this
// program keeps its own launch loop, which sets lcp_grid; EXPECT, the blocks and the reference come from check_common.hpp.  The
// text, the suffix array and every scratch array are heap blocks of exactly the size the library carves, so a read or
// write one element outside any of them stops the run.  What it walks:
//   - a few hundred random small texts (alphabets 1, 2, 4, 256; lengths 1 .. 300; short caps 16, 32 and 256, so that the
//     long-item kernel runs too) against suffixes sorted and compared directly, and the summary against a plain loop;
//   - suffix arrays with an entry above n (in row 0, in the middle, in the last row), with a value twice (one missing),
//     with row 0 repeated: the flag must be raised, and nothing out of bounds;
//   - wrong permutations (reversed, rotated, random): no flag required, every value within n - max(sa[j-1], sa[j]),
//     also with a long-item list of one slot, which such an array can overflow;
//   - planted pairs (a random block twice, one byte between) of 15 .. 14609 bytes, the second copy running to the end of
//     the text or stopping at a differing byte, at caps 16, 32, 48 and 256: the one-lane turn is 32 bytes, so the end of
//     the comparable bytes falls on every offset within a turn;
//   - the texts and arrays of tests/test_gpu_lcp_long.py (its part e: n = 1000 and 4097, the same generator): rows set
//     to n + 1 and 0xffffffff in row 0, the middle and the last row, a value twice, row 0's value repeated, the reversed
//     and a shuffled permutation -- walked here before the device sees them.
#define TC_LCP_HOST_CHECK
#include "tc_lcp.hpp"
#include "check_common.hpp"   // EXPECT, the blocks, the naive suffix array and the texts

template <class F>
static void launch(u32 grid, F &&kernel) {
    lcp_grid = grid;
    for (lcp_block = 0; lcp_block < grid; lcp_block++) kernel();
}
static u32 cdiv(u64 a, u64 b) { return (u32)((a + b - 1) / b); }

// the launch sequence of lcp_device; returns the error word
static u32 run_lcp(const std::vector<u8> &text, const std::vector<u32> &sa_in, u32 cap, u64 list_cap, std::vector<u32> &lcp_out) {
    const u32 n = (u32)text.size();
    const u64 N = (u64)n + 1;
    EXPECT(sa_in.size() == N);
    auto t = block_of(text);
    auto sa = block_of(sa_in);
    const u32 ntiles = cdiv(N, LCP_SCAN_TILE);
    // exactly N words: the scan's full-tile path must not pass N
    auto v = block<u32>(N);
    auto list = block<u32>(list_cap);
    auto tmax = block<u32>(ntiles);
    auto lcp = block<u32>(N);
    u32 count = 0, err = 0;
    std::memset(v.get(), 0xff, N * 4);
    const u32 grid = cdiv(N, LCP_NT);
    launch(grid, [&] { lcp_phi_kernel(sa.get(), N, n, v.get(), &err); });
    launch(grid, [&] { lcp_irreducible_kernel(t.get(), n, sa.get(), v.get(), cap, list.get(), (u32)list_cap, &count, &err); });
    launch(3, [&] { lcp_long_kernel(t.get(), n, v.get(), cap, list.get(), (u32)list_cap, &count); });
    launch(ntiles, [&] { lcp_scan_reduce_kernel(v.get(), N, tmax.get()); });
    launch(1, [&] { lcp_scan_tiles_kernel(tmax.get(), ntiles, cdiv(ntiles, LCP_SCAN_NT)); });
    launch(ntiles, [&] { lcp_scan_apply_kernel(v.get(), N, tmax.get()); });
    launch(grid, [&] { lcp_gather_kernel(sa.get(), N, n, v.get(), lcp.get()); });
    lcp_out.assign(lcp.get(), lcp.get() + N);
    return err;
}

static u64 list_cap_of(u64 n, u32 cap) {   // lcp_list_cap of csrc/tc_lcp_host.hpp
    int lg = 0;
    while (lg < 63 && (1ull << lg) < n + 1) lg++;
    const u64 bound = 2 * n * (u64)lg / cap + 1;
    return bound < n ? bound : n;
}

static void reference(const std::vector<u8> &text, std::vector<u32> &sa, std::vector<u32> &lcp) {
    sa = sort_suffixes(text);
    lcp = lcp_of(text, sa);
}

static void check_bounds(const std::vector<u32> &sa, const std::vector<u32> &lcp, u32 n) {
    EXPECT(lcp[0] == 0);
    for (u32 j = 1; j <= n; j++) {
        const u32 a = sa[j - 1], b = sa[j];
        if (a > n || b > n) EXPECT(lcp[j] == 0);
        else EXPECT(lcp[j] <= n - std::max(a, b));
    }
}

// the generator of tests/test_gpu_lcp_long.py (class Lcg), so that both walk the same texts and arrays
struct Lcg {
    u32 x;
    u32 next() {
        x = (u32)(((u64)x * 1103515245u + 12345u) & 0x7fffffffu);
        return x >> 16;
    }
};

// a random block of m bytes over 4 letters twice, '#' between; at_end: the text ends with the second copy, else '$' and
// five more letters follow
static std::vector<u8> planted_pair(std::mt19937_64 &rng, u32 m, bool at_end) {
    std::vector<u8> b(m), t;
    for (auto &c : b) c = (u8)"ACGT"[rng() % 4];
    t.insert(t.end(), b.begin(), b.end());
    t.push_back('#');
    t.insert(t.end(), b.begin(), b.end());
    if (!at_end) {
        t.push_back('$');
        for (int k = 0; k < 5; k++) t.push_back((u8)"ACGT"[rng() % 4]);
    }
    return t;
}

static u64 planted_pairs(std::mt19937_64 &rng) {
    const u32 lengths[] = {15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 256, 257, 272, 287, 288, 289, 1279, 2304, 6401, 14609};
    const u32 caps[] = {16, 32, 48, 256};
    u64 runs = 0;
    for (u32 m : lengths)
        for (int at_end = 0; at_end < 2; at_end++) {
            const std::vector<u8> text = planted_pair(rng, m, at_end != 0);
            std::vector<u32> sa, want, got;
            reference(text, sa, want);
            EXPECT(*std::max_element(want.begin(), want.end()) == m);
            for (u32 cap : caps) {
                EXPECT(run_lcp(text, sa, cap, list_cap_of(text.size(), cap), got) == 0);
                EXPECT(got == want);
                runs++;
            }
        }
    return runs;
}

// part e of tests/test_gpu_lcp_long.py: the same text, the same arrays
static u64 malformed_as_the_device_test(u32 n) {
    Lcg g{n};
    std::vector<u8> text(n);
    for (auto &c : text) c = (u8)(65 + (g.next() & 1));
    for (u32 k = 0; k < 300; k++) text[n / 2 + k] = text[k];
    std::vector<u32> sa, want, got, bad;
    reference(text, sa, want);
    u64 arrays = 0;
    for (u32 cap : {256u, 16u}) {
        const u64 lc = list_cap_of(n, cap);
        EXPECT(run_lcp(text, sa, cap, lc, got) == 0);
        EXPECT(got == want);
        for (u32 where : {0u, n / 2, n})
            for (u32 value : {n + 1, 0xffffffffu}) {
                bad = sa;
                bad[where] = value;
                EXPECT(run_lcp(text, bad, cap, lc, got) & LCP_ERR_SA);
                check_bounds(bad, got, n);
                arrays++;
            }
        bad = sa;
        bad[n / 3] = sa[2 * n / 3];
        EXPECT(run_lcp(text, bad, cap, lc, got) & LCP_ERR_SA);
        check_bounds(bad, got, n);
        bad = sa;
        bad[n / 2 + 1] = sa[0];
        EXPECT(run_lcp(text, bad, cap, lc, got) & LCP_ERR_SA);
        check_bounds(bad, got, n);
        // the two permutations must come back WITHOUT the flag: the device test expects a result from them
        bad = sa;
        std::reverse(bad.begin(), bad.end());
        EXPECT(run_lcp(text, bad, cap, lc, got) == 0);
        check_bounds(bad, got, n);
        bad = sa;
        Lcg h{n + 1};
        for (u32 i = n; i > 0; i--) std::swap(bad[i], bad[h.next() % (i + 1)]);
        EXPECT(run_lcp(text, bad, cap, lc, got) == 0);
        check_bounds(bad, got, n);
        arrays += 4;
    }
    return arrays;
}

int main() {
    std::mt19937_64 rng(0x1C9);
    const u32 alphabets[] = {1, 2, 4, 256};
    const u32 caps[] = {16, 32, 256};
    u64 texts = 0, long_runs = 0;
    for (int rep = 0; rep < 400; rep++) {
        const u32 sigma = alphabets[rep % 4];
        const u32 n = 1 + (u32)(rng() % (rep % 5 == 0 ? 300 : 70));
        std::vector<u8> text(n);
        for (auto &c : text) c = sigma == 256 ? (u8)rng() : (u8)(rng() % sigma ? 255 - rng() % sigma : 0);
        if (rep % 7 == 0)   // a repeat longer than the caps
            for (u32 i = n / 2; i < n; i++) text[i] = text[i - n / 2];
        std::vector<u32> sa, want, got;
        reference(text, sa, want);
        for (u32 cap : caps) {
            const u64 lc = list_cap_of(n, cap);
            EXPECT(run_lcp(text, sa, cap, lc, got) == 0);
            EXPECT(got == want);
            if (*std::max_element(want.begin(), want.end()) >= cap) long_runs++;
        }
        // the summary, over an odd number of workgroups
        u64 out2[2] = {0, 0};
        launch(3, [&] { lcp_summary_kernel(want.data(), (u64)n + 1, out2); });
        u64 sum = 0;
        u32 mx = 0, row = 0;
        for (u32 j = 0; j <= n; j++) {
            sum += want[j];
            if (want[j] > mx) { mx = want[j]; row = j; }
        }
        EXPECT((u32)(out2[0] >> 32) == mx && 0xffffffffu - (u32)out2[0] == row && out2[1] == sum);
        texts++;

        // ---- suffix arrays that are none
        const u32 cap = caps[rep % 3];
        const u64 lc = list_cap_of(n, cap);
        std::vector<u32> bad;
        const u32 above[] = {n + 1, 0x7fffffffu, 0xffffffffu};
        for (u32 where : {0u, n / 2, n}) {
            bad = sa;
            bad[where] = above[rep % 3];
            EXPECT(run_lcp(text, bad, cap, lc, got) & LCP_ERR_SA);
            check_bounds(bad, got, n);
        }
        if (n >= 2) {
            bad = sa;
            bad[1 + rng() % n] = sa[1 + rng() % n];   // maybe a duplicate ...
            bad[n] = bad[1];                                                     // ... certainly one when n >= 2
            if (bad != sa) {
                std::vector<u32> seen(n + 1, 0);
                bool perm = true;
                for (u32 x : bad) perm = perm && x <= n && !seen[x]++;
                if (!perm) {
                    EXPECT(run_lcp(text, bad, cap, lc, got) & LCP_ERR_SA);
                    check_bounds(bad, got, n);
                }
            }
            bad = sa;
            bad[n / 2 + 1 > n ? n : n / 2 + 1] = sa[0];   // row 0's value twice, another missing
            EXPECT(run_lcp(text, bad, cap, lc, got) & LCP_ERR_SA);
            check_bounds(bad, got, n);
            // ---- permutations that are not this text's suffix array
            bad = sa;
            std::reverse(bad.begin(), bad.end());
            (void)run_lcp(text, bad, cap, lc, got);
            check_bounds(bad, got, n);
            bad = sa;
            std::rotate(bad.begin(), bad.begin() + 1, bad.end());
            (void)run_lcp(text, bad, cap, 1, got);
            check_bounds(bad, got, n);
            for (u32 i = 0; i <= n; i++) bad[i] = i;   // identity: phi[i] = i - 1, every comparison runs to the end of the text
            (void)run_lcp(text, bad, 16, 1, got);
            check_bounds(bad, got, n);
            std::shuffle(bad.begin(), bad.end(), rng);
            (void)run_lcp(text, bad, cap, lc, got);
            check_bounds(bad, got, n);
        }
    }
    EXPECT(long_runs > 20);
    const u64 pair_runs = planted_pairs(rng);
    const u64 arrays = malformed_as_the_device_test(1000) + malformed_as_the_device_test(4097);
    std::printf("lcp kernels: %llu texts x 3 caps exact (%llu runs with long items), %llu runs of planted pairs exact, malformed and "
                "wrong suffix arrays in bounds (%llu of them the device test's)\n",
                (unsigned long long)texts, (unsigned long long)long_runs, (unsigned long long)pair_runs, (unsigned long long)arrays);
    return 0;
}
