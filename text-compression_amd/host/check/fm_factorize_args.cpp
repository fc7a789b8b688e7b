// Stand-alone host check of the argument and capacity handling of tc_fm_factorize / tc_fm_unfactorize, meant to be built
// with a host sanitizer together with the library's host code:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -pthread -Xarch_host -fsanitize=address,undefined \
//         -I include -I text-compression_amd/csrc text-compression_amd/csrc/textcomp.hip \
//         text-compression_amd/host/check/fm_factorize_args.cpp -o fm_factorize_args && ./fm_factorize_args
// It packs a few patterns and walks every path that returns before a kernel is launched: a null context, a null index, a
// null capacity word, null buffers, one payload array without the other, npat = 0, unfactorize on an index without text
// samples -- with a capacity one short of what a real batch would need, so the capacity word is read and written on every
// path.  With a device present it goes on to a real call: the empty index (every byte a literal), the sizes-only form,
// capacity one short (TC_ERR_CAPACITY, the total, nothing written), exactly enough, the round trip through
// tc_fm_unfactorize, and a bad factor list.  Without one, tc_ctx_create fails and the check ends after the calls that need
// no context (exit 0, and it says so).
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
    const std::vector<std::string> pats = {"ACGTACXTTGA", "TTGA", "", "ZACGZ"};
    std::string flat;
    std::vector<uint64_t> offs(1, 0);
    for (const auto &p : pats) {
        flat += p;
        offs.push_back(flat.size());
    }
    const uint64_t nbytes_all = flat.size();
    flat.push_back('\0');
    const uint8_t *fp = reinterpret_cast<const uint8_t *>(flat.data());
    const uint64_t npat = pats.size();
    std::vector<uint64_t> foffs(npat + 1, 7), fpos(32, 7), ooffs(npat + 1, 7);
    std::vector<uint32_t> flen(32, 7);
    std::vector<uint8_t> out(64, 7);
    uint64_t nf = fpos.size() - 1, nb = out.size() - 1;

    // no context: refused before anything is touched
    EXPECT(tc_fm_factorize(nullptr, nullptr, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_ERR_ARG);
    EXPECT(tc_fm_factorize_dev(nullptr, nullptr, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_ERR_ARG);
    EXPECT(tc_fm_unfactorize(nullptr, nullptr, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_ARG);
    EXPECT(tc_fm_unfactorize_dev(nullptr, nullptr, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_ARG);
    EXPECT(nf == fpos.size() - 1 && nb == out.size() - 1 && foffs[0] == 7 && fpos[0] == 7 && out[0] == 7);

    tc_ctx *ctx = nullptr;
    if (tc_ctx_create(0, &ctx) != TC_OK) {
        std::printf("no device: checked the calls that need no context (4 entry points, null context)\n");
        return 0;
    }
    tc_fm *empty = nullptr;
    EXPECT(tc_fm_build(ctx, nullptr, 0, &empty) == TC_OK && empty);
    // a null index, a null capacity word, null buffers, one payload array without the other, npat = 0
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, nullptr, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_ERR_ARG);
    EXPECT(tc_fm_factorize(ctx, empty, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), nullptr) == TC_ERR_ARG);
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, empty, nullptr, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_ERR_ARG && nf == 0);
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, empty, fp, offs.data(), npat, nullptr, fpos.data(), flen.data(), &nf) == TC_ERR_ARG);
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, empty, fp, offs.data(), npat, foffs.data(), fpos.data(), nullptr, &nf) == TC_ERR_ARG);
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, empty, fp, offs.data(), npat, foffs.data(), nullptr, nullptr, &nf) == TC_ERR_ARG);   // (a capacity, no arrays)
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, empty, fp, offs.data(), 0, nullptr, nullptr, nullptr, &nf) == TC_OK && nf == 0);
    nb = 63;
    EXPECT(tc_fm_unfactorize(ctx, nullptr, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_ARG);
    EXPECT(tc_fm_unfactorize(ctx, empty, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), nullptr) == TC_ERR_ARG);
    nb = 63;
    EXPECT(tc_fm_unfactorize(ctx, empty, foffs.data(), fpos.data(), flen.data(), 0, ooffs.data(), nullptr, &nb) == TC_OK && nb == 0 && ooffs[0] == 0);
    nb = 63;        // the empty index holds no text samples
    EXPECT(tc_fm_unfactorize(ctx, empty, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_ARG && nb == 0);
    EXPECT(foffs[0] == 7 && fpos[0] == 7 && flen[0] == 7 && out[0] == 7);

    // the empty index: every byte is a literal
    nf = 31;
    EXPECT(tc_fm_factorize(ctx, empty, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_OK && nf == nbytes_all);
    for (uint64_t p = 0; p <= npat; p++) EXPECT(foffs[p] == offs[p]);
    for (uint64_t f = 0; f < nf; f++) EXPECT(fpos[f] == fp[f] && flen[f] == 0);
    tc_fm_free(empty);

    // a real batch: sizes only, capacity one short, exactly enough
    const std::string text = "ACGTACGTTACGAACGTACTTGACG";
    tc_fm *fm = nullptr, *plain = nullptr;
    EXPECT(tc_fm_build_self(ctx, reinterpret_cast<const uint8_t *>(text.data()), text.size(), 4, 4, &fm) == TC_OK);
    EXPECT(tc_fm_build(ctx, reinterpret_cast<const uint8_t *>(text.data()), text.size(), &plain) == TC_OK);
    uint64_t total = 0;
    EXPECT(tc_fm_factorize(ctx, fm, fp, offs.data(), npat, foffs.data(), nullptr, nullptr, &total) == TC_OK);
    EXPECT(total > 1 && total <= 31 && foffs[0] == 0 && foffs[npat] == total && foffs[2] == foffs[3]);
    fpos.assign(total, 7);
    flen.assign(total, 7);
    nf = total - 1;
    EXPECT(tc_fm_factorize(ctx, fm, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_ERR_CAPACITY);
    EXPECT(nf == total && fpos[0] == 7 && flen[0] == 7);
    EXPECT(tc_fm_factorize(ctx, fm, fp, offs.data(), npat, foffs.data(), fpos.data(), flen.data(), &nf) == TC_OK);
    EXPECT(nf == total && foffs[npat] == total);
    for (uint64_t f = 0; f < total; f++)        // a match lies in the text; the literals are the X and the two Z
        EXPECT(flen[f] ? (fpos[f] >= 1 && fpos[f] - 1 + flen[f] <= text.size()) : (fpos[f] == 'X' || fpos[f] == 'Z'));
    {   // the sampled index and the full one answer alike
        std::vector<uint64_t> o2(npat + 1), p2(total);
        std::vector<uint32_t> l2(total);
        uint64_t n2 = total;
        EXPECT(tc_fm_factorize(ctx, plain, fp, offs.data(), npat, o2.data(), p2.data(), l2.data(), &n2) == TC_OK && n2 == total);
        EXPECT(o2 == foffs && p2 == fpos && l2 == flen);
    }
    // the round trip: capacity one short, then exactly enough
    out.assign(nbytes_all, 7);
    nb = nbytes_all - 1;
    EXPECT(tc_fm_unfactorize(ctx, fm, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_CAPACITY);
    EXPECT(nb == nbytes_all && out[0] == 7);
    EXPECT(tc_fm_unfactorize(ctx, fm, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_OK);
    EXPECT(nb == nbytes_all && std::memcmp(out.data(), fp, nbytes_all) == 0);
    for (uint64_t p = 0; p <= npat; p++) EXPECT(ooffs[p] == offs[p]);
    // an index without text samples; a bad list (a match over the end of the text): nothing written
    nb = nbytes_all;
    EXPECT(tc_fm_unfactorize(ctx, plain, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_ARG);
    out.assign(nbytes_all, 7);
    fpos[0] = text.size();
    flen[0] = 2;
    nb = nbytes_all;
    EXPECT(tc_fm_unfactorize(ctx, fm, foffs.data(), fpos.data(), flen.data(), npat, ooffs.data(), out.data(), &nb) == TC_ERR_ARG);
    EXPECT(out[0] == 7);
    tc_fm_free(fm);
    tc_fm_free(plain);
    tc_ctx_destroy(ctx);
    std::printf("ok: argument, capacity, factorize and unfactorize paths\n");
    return 0;
}
