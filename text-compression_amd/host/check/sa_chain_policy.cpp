// Stand-alone host check of ChainPolicy (csrc/tc_sa_plan.hpp): when a doubling round of the suffix sort becomes a chain
// round.  No device and no HIP header; meant to be built with a host sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I text-compression_amd/csrc
//       text-compression_amd/host/check/sa_chain_policy.cpp -o sa_chain_policy && ./sa_chain_policy
// The expectations are what the comment on ChainPolicy promises (and tests/test_gpu_chain.py sees on the device): no
// chain in the first doubling round; one after a plain round that shed less than 1/256 of at least 2^20 members; its
// second pass keeps h; a chain round that resolved less than an eighth makes the next attempt wait 2, then 4 plain
// rounds, and after three such rounds there are none; TC_SA_CHAIN=2 ignores the back-off, 0 never chains.

static int env_int(const char *, int dflt) { return dflt; }   // (the knobs at their defaults, whatever the environment)
#include "tc_sa_plan.hpp"
#include "check_common.hpp"   // EXPECT

static const uint64_t N = 1ull << 24;

// a plain round at depth h over m members that sheds next to nothing (one member); true if it was offered as a chain
// round's start and taken -- then nothing else is done
static bool plain_round_or_chain(ChainPolicy &c, uint64_t &h, uint64_t &m) {
    if (c.start(true, (uint32_t)h, h, N, m)) return true;
    if (c.finish(m, m - 1)) h *= 2;
    m -= 1;
    return false;
}
// both passes of a chain round that was just started, leaving m_left members tied
static int chain_round(ChainPolicy &c, uint64_t &h, uint64_t &m, uint64_t m_left) {
    const uint64_t h0 = h;
    EXPECT(c.keymode == 1);
    EXPECT(!c.finish(m, m - 1));              // the first pass: the second one keeps h
    EXPECT(c.keymode == 2 && h == h0);
    EXPECT(!c.start(true, (uint32_t)h, h, N, m - 1));   // (no chain round inside a chain round)
    EXPECT(c.finish(m - 1, m_left));          // the second pass: h doubles
    EXPECT(c.keymode == 0);
    h *= 2;
    m = m_left;
    return 0;
}

int main() {
    const uint64_t M = 1ull << 22;
    {   // the default policy
        ChainPolicy c(SaKnobs{}.chain);
        EXPECT(c.mode == 1);
        uint64_t h = 21, m = M;
        EXPECT(!plain_round_or_chain(c, h, m));    // never in the first doubling round, however little round 0 resolved
        EXPECT(h == 42);
        EXPECT(plain_round_or_chain(c, h, m));     // the plain round shed 1 of 2^22: a chain round starts
        EXPECT(chain_round(c, h, m, 5) == 0);      // ... and resolves nearly everything: no back-off
        EXPECT(h == 84 && c.chain_fail == 0 && c.chain_wait == 0);
    }
    {   // what does not start one: a set below 2^20, a round that shed 1/256 or more, a radix round, h < 4, h >= N
        ChainPolicy c(1);
        EXPECT(c.finish(M, M - M / 256));          // a plain round that shed exactly 1/256
        EXPECT(!c.start(true, 42, 42, N, M - M / 256));
        EXPECT(c.finish(M, M - M / 256 + 1));      // just under 1/256
        EXPECT(!c.start(false, 42, 42, N, M - M / 256 + 1));
        EXPECT(!c.start(true, 3, 3, N, M - M / 256 + 1));
        EXPECT(!c.start(true, (uint32_t)N, N, N, M - M / 256 + 1));
        EXPECT(c.start(true, 42, 42, N, M - M / 256 + 1));
        ChainPolicy d(1);
        EXPECT(d.finish((1u << 20) - 1, (1u << 20) - 2));
        EXPECT(!d.start(true, 42, 42, N, (1u << 20) - 2));   // fewer than 2^20 members
        EXPECT(d.finish(1u << 20, 1u << 20));
        EXPECT(d.start(true, 42, 42, N, 1u << 20));
    }
    {   // back-off: chain rounds that resolve less than an eighth
        ChainPolicy c(1);
        uint64_t h = 4, m = 1ull << 23;
        EXPECT(!plain_round_or_chain(c, h, m));
        for (int fail = 1; fail <= 3; fail++) {
            EXPECT(plain_round_or_chain(c, h, m));
            EXPECT(chain_round(c, h, m, m - m / 8 + 8) == 0);   // resolved just under an eighth
            EXPECT(c.chain_fail == fail);
            if (fail == 3) break;
            // the next attempt waits 2, then 4 plain rounds
            for (int r = 0; r < (1 << fail); r++) EXPECT(!plain_round_or_chain(c, h, m));
        }
        for (int r = 0; r < 12; r++) EXPECT(!plain_round_or_chain(c, h, m));   // after three failures: no more
        EXPECT(m >= (1u << 20));   // (the set stayed above the trigger's floor all along)
    }
    {   // a chain round that resolves an eighth or more does not count as a failure
        ChainPolicy c(1);
        uint64_t h = 4, m = 1ull << 23;
        EXPECT(!plain_round_or_chain(c, h, m));
        EXPECT(plain_round_or_chain(c, h, m));
        EXPECT(chain_round(c, h, m, m - 1 - (m + 7) / 8) == 0);
        EXPECT(c.chain_fail == 0 && c.chain_wait == 0);
        EXPECT(!plain_round_or_chain(c, h, m));    // (a chain round came since the last plain round)
        EXPECT(plain_round_or_chain(c, h, m));
    }
    {   // TC_SA_CHAIN=2: every segmented round, the first one and small sets included, whatever failed before
        ChainPolicy c(2);
        uint64_t h = 4, m = 70000;
        for (int r = 0; r < 6; r++) {
            EXPECT(plain_round_or_chain(c, h, m));
            EXPECT(chain_round(c, h, m, m - 2) == 0);
        }
        EXPECT(!c.start(false, (uint32_t)h, h, N, m));   // (but only a segmented round can)
    }
    {   // TC_SA_CHAIN=0: never
        ChainPolicy c(0);
        uint64_t h = 4, m = M;
        for (int r = 0; r < 8; r++) EXPECT(!plain_round_or_chain(c, h, m));
    }
    std::printf("ok: chain-round policy\n");
    return 0;
}
