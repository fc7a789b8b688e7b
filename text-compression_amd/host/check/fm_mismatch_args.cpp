// Stand-alone host check of the argument and capacity handling of tc_fm_count_mm / tc_fm_locate_mm, meant to be built
// with a host sanitizer together with the library's host code:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -pthread -Xarch_host -fsanitize=address,undefined \
//         -I include -I text-compression_amd/csrc text-compression_amd/csrc/textcomp.hip \
//         text-compression_amd/host/check/fm_mismatch_args.cpp -o fm_mismatch_args && ./fm_mismatch_args
// It packs a few patterns and walks every path that returns before a kernel is launched: a null context, a null index,
// k above TC_FM_MAX_MISMATCH, null buffers, npat = 0, the empty index (zeros; *nhits is reset) -- with a hit capacity one
// short of what a real batch would need, so the capacity word is read and written on every path.  With a device present it
// goes on to a real search: capacity one short (TC_ERR_CAPACITY, the total, nothing written), then exactly enough.
// Without one, tc_ctx_create fails and the check ends after the calls that need no context (exit 0, and it says so).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "textcomp.h"

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

int main() {
    const std::vector<std::string> pats = {"ACGTAC", "TTGA", "", "ACG"};
    std::string flat;
    std::vector<uint64_t> offs(1, 0);
    for (const auto &p : pats) {
        flat += p;
        offs.push_back(flat.size());
    }
    flat.push_back('\0');
    const uint8_t *fp = reinterpret_cast<const uint8_t *>(flat.data());
    const uint64_t npat = pats.size();
    std::vector<int64_t> cnt(npat, -1);
    std::vector<uint64_t> hoffs(npat + 1, 7), hits(16, 7);
    std::vector<uint8_t> mm(16, 7);
    uint64_t nh = hits.size() - 1;

    // no context: refused before anything is touched
    EXPECT(tc_fm_count_mm(nullptr, nullptr, fp, offs.data(), npat, 1, cnt.data()) == TC_ERR_ARG);
    EXPECT(tc_fm_count_mm_dev(nullptr, nullptr, fp, offs.data(), npat, 1, cnt.data()) == TC_ERR_ARG);
    EXPECT(tc_fm_locate_mm(nullptr, nullptr, fp, offs.data(), npat, 1, hoffs.data(), hits.data(), mm.data(), &nh) == TC_ERR_ARG);
    EXPECT(tc_fm_locate_mm_dev(nullptr, nullptr, fp, offs.data(), npat, 1, hoffs.data(), hits.data(), mm.data(), &nh) == TC_ERR_ARG);
    EXPECT(nh == hits.size() - 1 && cnt[0] == -1 && hits[0] == 7);

    tc_ctx *ctx = nullptr;
    if (tc_ctx_create(0, &ctx) != TC_OK) {
        std::printf("no device: checked the calls that need no context (4 entry points, null context)\n");
        return 0;
    }
    tc_fm *empty = nullptr;
    EXPECT(tc_fm_build(ctx, nullptr, 0, &empty) == TC_OK && empty);
    // a null index, k too large, null buffers, npat = 0
    EXPECT(tc_fm_count_mm(ctx, nullptr, fp, offs.data(), npat, 1, cnt.data()) == TC_ERR_ARG);
    EXPECT(tc_fm_count_mm(ctx, empty, fp, offs.data(), npat, TC_FM_MAX_MISMATCH + 1, cnt.data()) == TC_ERR_ARG);
    EXPECT(tc_fm_count_mm(ctx, empty, nullptr, offs.data(), npat, 1, cnt.data()) == TC_ERR_ARG);
    EXPECT(tc_fm_count_mm(ctx, empty, fp, offs.data(), 0, 1, nullptr) == TC_OK);
    nh = 15;
    EXPECT(tc_fm_locate_mm(ctx, nullptr, fp, offs.data(), npat, 1, hoffs.data(), hits.data(), mm.data(), &nh) == TC_ERR_ARG);
    nh = 15;
    EXPECT(tc_fm_locate_mm(ctx, empty, fp, offs.data(), npat, TC_FM_MAX_MISMATCH + 1, hoffs.data(), hits.data(), mm.data(), &nh) == TC_ERR_ARG && nh == 0);
    nh = 15;
    EXPECT(tc_fm_locate_mm(ctx, empty, fp, offs.data(), npat, 1, nullptr, hits.data(), mm.data(), &nh) == TC_ERR_ARG);
    EXPECT(tc_fm_locate_mm(ctx, empty, fp, offs.data(), npat, 1, hoffs.data(), hits.data(), mm.data(), nullptr) == TC_ERR_ARG);
    nh = 15;
    EXPECT(tc_fm_locate_mm(ctx, empty, fp, offs.data(), 0, 1, nullptr, nullptr, nullptr, &nh) == TC_OK && nh == 0);
    // the empty index answers zeros
    EXPECT(tc_fm_count_mm(ctx, empty, fp, offs.data(), npat, 3, cnt.data()) == TC_OK);
    for (int64_t c : cnt) EXPECT(c == 0);
    nh = 15;
    EXPECT(tc_fm_locate_mm(ctx, empty, fp, offs.data(), npat, 3, hoffs.data(), hits.data(), nullptr, &nh) == TC_OK && nh == 0);
    for (uint64_t o : hoffs) EXPECT(o == 0);
    tc_fm_free(empty);

    // a real batch: capacity one short, then exactly enough
    const std::string text = "ACGTACGTTACGAACGTACTTGACG";
    tc_fm *fm = nullptr;
    EXPECT(tc_fm_build(ctx, reinterpret_cast<const uint8_t *>(text.data()), text.size(), &fm) == TC_OK);
    EXPECT(tc_fm_count_mm(ctx, fm, fp, offs.data(), npat, 1, cnt.data()) == TC_OK);
    uint64_t total = 0;
    for (int64_t c : cnt) total += (uint64_t)c;
    EXPECT(total > 1);
    hits.assign(total, 7);
    mm.assign(total, 7);
    nh = total - 1;
    EXPECT(tc_fm_locate_mm(ctx, fm, fp, offs.data(), npat, 1, hoffs.data(), hits.data(), mm.data(), &nh) == TC_ERR_CAPACITY);
    EXPECT(nh == total && hits[0] == 7 && mm[0] == 7);
    EXPECT(tc_fm_locate_mm(ctx, fm, fp, offs.data(), npat, 1, hoffs.data(), hits.data(), mm.data(), &nh) == TC_OK);
    EXPECT(nh == total && hoffs[npat] == total);
    for (uint64_t h = 0; h < total; h++) EXPECT(hits[h] >= 1 && hits[h] <= text.size() && mm[h] <= 1);
    tc_fm_free(fm);
    tc_ctx_destroy(ctx);
    std::printf("ok: argument, capacity and search paths\n");
    return 0;
}
