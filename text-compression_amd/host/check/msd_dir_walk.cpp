// Stand-alone host check of the aligned MSD level's tile cursor over a directory of live parents (csrc/tc_msd_dir.hpp)
// against a transcription of the walk it replaces (csrc/tc_msd.hpp: msd_cur_init / msd_cur_info over tpre, pstart, pcnt).
// No device and no HIP header; meant to be built with a host sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/msd_dir_walk.cpp -o msd_dir_walk && ./msd_dir_walk
// For every table and every (capacity, batch) the two walks must give the same tiles -- base, valid, q, last -- in the
// same order, the protocol around the cursor must hold (msd_dir_walk's `bad`), and the fills must be what the table
// implies where that is easy to say.

#include "tc_msd_dir.hpp"
#include "check_common.hpp"   // EXPECT

static const uint32_t TILE = 8192;

// ---- the old walk, transcribed (tile numbers from tpre; thread 0's cursor) ------------------------------------------
struct OldLevel {
    const uint32_t *pstart, *pcnt, *tpre;
    uint32_t nparents;
};
static uint32_t old_find_parent(const uint32_t *tpre, uint32_t nparents, uint32_t t) {
    uint32_t lo = 0, hi = nparents;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tpre[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
struct OldCur {
    uint32_t q, tq0, tq1, ps, pc;
};
static void old_cur_init(const OldLevel &L, OldCur &c, uint32_t t) {
    c.q = old_find_parent(L.tpre, L.nparents, t);
    c.tq0 = L.tpre[c.q]; c.tq1 = L.tpre[c.q + 1]; c.ps = L.pstart[c.q]; c.pc = L.pcnt[c.q];
}
static void old_cur_info(const OldLevel &L, OldCur &c, uint32_t t, uint32_t t_end, MsdDirTile *out) {
    if (t >= t_end) {
        out->base = 0; out->valid = 0; out->q = 0; out->last = 0;
        return;
    }
    if (t >= c.tq1) {
        uint32_t q = c.q + 1;
        while (L.tpre[q + 1] <= t) q++;
        c.q = q; c.tq0 = L.tpre[q]; c.tq1 = L.tpre[q + 1]; c.ps = L.pstart[q]; c.pc = L.pcnt[q];
    }
    const uint32_t off = (t - c.tq0) * TILE;
    out->base = c.ps + off;
    out->valid = c.pc - off < TILE ? c.pc - off : TILE;
    out->q = c.q;
    out->last = (t + 1 >= t_end || t + 1 >= c.tq1) ? 1u : 0u;
}

// a table of parent counts -> pstart, tpre; the slots [q0, q1) walked both ways with directory capacity `cap`
struct Table {
    std::vector<uint32_t> pcnt, pstart, tpre;
    explicit Table(const std::vector<uint32_t> &c) : pcnt(c), pstart(c.size()), tpre(c.size() + 1) {
        uint32_t pos = 0, t = 0;
        for (size_t q = 0; q < c.size(); q++) {
            pstart[q] = pos; tpre[q] = t;
            pos += c[q]; t += (c[q] + TILE - 1) / TILE;
        }
        tpre[c.size()] = t;
    }
};
static int compare(const Table &T, uint32_t q0, uint32_t q1, uint32_t cap, uint32_t batch, uint32_t *fills_out) {
    const OldLevel L = {T.pstart.data(), T.pcnt.data(), T.tpre.data(), (uint32_t)T.pcnt.size()};
    const uint32_t t0 = T.tpre[q0], t1 = T.tpre[q1];
    std::vector<MsdDirTile> want;
    if (t0 < t1) {   // (the kernel returns before it makes a cursor when the workgroup has no tile)
        OldCur c;
        old_cur_init(L, c, t0);
        for (uint32_t t = t0; t < t1; t++) {
            MsdDirTile d;
            old_cur_info(L, c, t, t1, &d);
            want.push_back(d);
        }
    }
    std::vector<MsdDirEnt> dir(cap);   // exactly cap entries: ASan sees a write past the capacity
    std::vector<MsdDirTile> got(want.size() + 4);
    uint32_t fills = 0;
    int bad = 0;
    const uint64_t n = msd_dir_walk(T.pcnt.data(), T.pstart.data(), q0, q1, dir.data(), cap, batch, TILE, got.data(), got.size(),
                                    &fills, &bad);
    EXPECT(!bad);
    EXPECT(n == want.size());
    for (size_t i = 0; i < want.size(); i++) {
        EXPECT(got[i].base == want[i].base);
        EXPECT(got[i].valid == want[i].valid);
        EXPECT(got[i].q == want[i].q);
        EXPECT(got[i].last == want[i].last);
    }
    if (fills_out) *fills_out = fills;
    return 0;
}
// every (capacity, batch) the kernel uses and some it does not, over the whole table and over inner slot ranges
static int sweep(const std::vector<uint32_t> &cnt) {
    const Table T(cnt);
    const uint32_t np = (uint32_t)cnt.size();
    const uint32_t caps[] = {1, 2, 3, 128, 1024}, batches[] = {1, 7, 1024};
    for (uint32_t cap : caps)
        for (uint32_t batch : batches) {
            if (compare(T, 0, np, cap, batch, nullptr)) return 1;
            if (np >= 4 && compare(T, np / 4, np - np / 4, cap, batch, nullptr)) return 1;
            if (np >= 2 && compare(T, 1, np, cap, batch, nullptr)) return 1;
        }
    return 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

int main() {
    uint32_t fills = 0;
    // no live parent (one slot, many slots); an empty slot range
    EXPECT(!sweep({0}));
    EXPECT(!sweep(std::vector<uint32_t>(3000, 0)));
    {
        const Table T(std::vector<uint32_t>(10, 5));
        EXPECT(!compare(T, 4, 4, 8, 1024, &fills));
        EXPECT(fills == 0);
    }
    // one live parent: alone, first, last, in the middle
    for (uint32_t pc : {1u, 8191u, 8192u, 8193u, 3u * 8192u, 3u * 8192u + 1u, 100000u}) {
        EXPECT(!sweep({pc}));
        std::vector<uint32_t> a(2500, 0), b(2500, 0), c(2500, 0);
        a[0] = pc; b[2499] = pc; c[1234] = pc;
        EXPECT(!sweep(a)); EXPECT(!sweep(b)); EXPECT(!sweep(c));
    }
    // live parents only at both ends of the range
    {
        std::vector<uint32_t> a(5000, 0);
        a[0] = 20000; a[4999] = 7;
        EXPECT(!sweep(a));
        const Table T(a);
        EXPECT(!compare(T, 0, 5000, 1024, 1024, &fills));
        EXPECT(fills == 1 + 4);   // the first round finds slot 0; the refill needs four rounds to reach slot 4999
    }
    // the counts around a tile, side by side
    EXPECT(!sweep({1, 8191, 8192, 8193, 3 * 8192, 0, 0, 1, 0, 8193}));
    // runs of one-tile parents: the look-ahead crosses three boundaries at every tile
    EXPECT(!sweep(std::vector<uint32_t>(300, 6)));
    EXPECT(!sweep(std::vector<uint32_t>(300, 8192)));
    {
        std::vector<uint32_t> a;
        for (int i = 0; i < 400; i++) { a.push_back(1 + i % 3); a.push_back(0); a.push_back(i % 5 == 0 ? 20000 : 0); }
        EXPECT(!sweep(a));
    }
    // more slots than the capacity holds, all live: fills = ceil(live / cap) when a batch covers everything
    {
        const Table T(std::vector<uint32_t>(1000, 9000));
        EXPECT(!compare(T, 0, 1000, 128, 1024, &fills));
        EXPECT(fills == 8);
        EXPECT(!compare(T, 0, 1000, 1, 1024, &fills));   // capacity 1: a fill per parent
        EXPECT(fills == 1000);
        EXPECT(!compare(T, 0, 1000, 1024, 1024, &fills));
        EXPECT(fills == 1);
    }
    // a refill that finds nothing live: the slots behind the last live parent are looked at and the walk ends
    {
        std::vector<uint32_t> a(4096, 0);
        a[10] = 30000;
        const Table T(a);
        EXPECT(!compare(T, 0, 4096, 1024, 1024, &fills));
        EXPECT(fills == 1 + 3);
        EXPECT(!sweep(a));
    }
    // a few thousand random tables: sparse and dense, small and large counts
    for (int it = 0; it < 3000; it++) {
        const uint32_t np = 1 + rnd() % 600, dens = 1 + rnd() % 8, big = rnd() % 4;
        std::vector<uint32_t> a(np);
        for (uint32_t q = 0; q < np; q++) {
            if (rnd() % dens) { a[q] = 0; continue; }
            switch (big ? rnd() % 4 : 0) {
            case 0: a[q] = 1 + rnd() % 40; break;
            case 1: a[q] = 8190 + rnd() % 5; break;
            case 2: a[q] = 1 + rnd() % 70000; break;
            default: a[q] = TILE * (1 + rnd() % 4); break;
            }
        }
        const Table T(a);
        const uint32_t x = rnd() % (np + 1), y = rnd() % (np + 1);
        const uint32_t q0 = x < y ? x : y, q1 = x < y ? y : x;
        const uint32_t cap = (it & 1) ? 1 + rnd() % 5 : (it & 2) ? 128 : 1024, batch = (it & 4) ? 1024 : 1 + rnd() % 64;
        EXPECT(!compare(T, q0, q1, cap, batch, nullptr));
        EXPECT(!compare(T, 0, np, cap, batch, nullptr));
    }
    std::printf("ok: directory walk of the aligned MSD level\n");
    return 0;
}
