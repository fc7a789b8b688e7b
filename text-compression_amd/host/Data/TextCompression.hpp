// TextCompression.hpp -- C++ host-side mirror of the reference's L3 module surface
// (Data.BWT / Data.MTF / Data.RLE / Data.FMIndex, ByteString instantiation) over the C ABI
// of include/textcomp.h.  Header only; links against libtextcomp.so.
//
// The reference is Haskell and no GHC exists in this image, so this is the compiled-language
// host layer: same function names, same argument meaning, same value shapes and the same
// error behaviour (what throws in the reference throws here), so that host code and tests
// read like the reference's.  Value shapes:
//   Seq (Maybe Word8)        -> std::vector<std::optional<uint8_t>>      (BWT Word8)
//   Seq (Maybe ByteString)   -> std::vector<std::optional<std::string>>  (RLE ByteString, BWT ByteString)
//   MTF ByteString           -> struct MTF { indices; final list }
//   Seq (ByteString, Maybe Int) -> std::vector<std::pair<std::string, std::optional<int64_t>>>
#pragma once
#include <array>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "textcomp.h"

namespace Data {

struct TextCompError : std::runtime_error {
    int code;
    TextCompError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// one process-wide context on device 0 (tc_ctx = device + stream + workspace)
class Context {
  public:
    static tc_ctx *get() {
        static Context c;
        return c.ctx_;
    }
    static void check(int rc) {
        if (rc != TC_OK) throw TextCompError(rc, tc_last_error(get()));
    }
    // what the context's container writers put behind the header: TC_CODING_PACKED (default) or TC_CODING_HUFFMAN
    static void setContainerCoding(int coding) { check(tc_ctx_set_container_coding(get(), coding)); }
    static int containerCoding() { return tc_ctx_get_container_coding(get()); }

  private:
    Context() {
        int rc = tc_ctx_create(0, &ctx_);
        if (rc != TC_OK) throw TextCompError(rc, "tc_ctx_create: no usable HIP device (there is no CPU fallback)");
    }
    ~Context() { tc_ctx_destroy(ctx_); }
    tc_ctx *ctx_ = nullptr;
};

using Word8Seq = std::vector<std::optional<uint8_t>>;
using BSSeq = std::vector<std::optional<std::string>>;

namespace detail {
inline std::vector<int16_t> toSym(const Word8Seq &s) {
    std::vector<int16_t> v(s.size());
    for (size_t i = 0; i < s.size(); i++) v[i] = s[i] ? (int16_t)*s[i] : (int16_t)-1;
    return v;
}
inline Word8Seq fromSym(const std::vector<int16_t> &v) {
    Word8Seq s(v.size());
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] >= 0) s[i] = (uint8_t)v[i];
    return s;
}
}  // namespace detail

namespace BWT {
// bytestringToBWT :: ByteString -> BWT Word8                              (BWT.hs:68-70)
inline Word8Seq bytestringToBWT(const std::string &bs) {
    if (bs.empty()) return {};  // BWT.hs:58
    std::vector<uint8_t> L(bs.size() + 1);
    uint64_t primary = 0;
    Context::check(tc_bwt_encode(Context::get(), (const uint8_t *)bs.data(), bs.size(), L.data(), &primary));
    Word8Seq out(L.size());
    for (size_t j = 0; j < L.size(); j++)
        if (j != primary) out[j] = L[j];
    return out;
}
// bytestringFromWord8BWT :: BWT Word8 -> ByteString                        (BWT.hs:108-110)
inline std::string bytestringFromWord8BWT(const Word8Seq &bwt) {
    if (bwt.empty()) return {};
    std::vector<int16_t> sym = detail::toSym(bwt);
    std::string out(bwt.size(), '\0');
    uint64_t n = 0;
    Context::check(tc_bwt_decode_sym(Context::get(), sym.data(), sym.size(), (uint8_t *)out.data(), &n));
    out.resize(n);
    return out;
}

// Not in the reference: the enhanced suffix array -- the suffix array (0-based starts, n + 1 rows, row 0 the empty
// suffix) and its LCP array (lcp[0] = 0; lcp[j] = longest common prefix of the suffixes at sa[j - 1] and sa[j]; the end
// of the text matches nothing) -- and what follows from it without a pattern.
struct EnhancedSuffixArray {
    std::vector<uint32_t> sa, lcp;
};
inline EnhancedSuffixArray bytestringToEnhancedSuffixArray(const std::string &bs) {
    EnhancedSuffixArray e;
    e.sa.resize(bs.size() + 1);
    e.lcp.resize(bs.size() + 1);
    Context::check(tc_lcp_array(Context::get(), (const uint8_t *)bs.data(), bs.size(), e.sa.data(), e.lcp.data()));
    return e;
}
inline std::vector<uint32_t> bytestringToLCPArray(const std::string &bs) {
    std::vector<uint32_t> lcp(bs.size() + 1);
    Context::check(tc_lcp_array(Context::get(), (const uint8_t *)bs.data(), bs.size(), nullptr, lcp.data()));
    return lcp;
}
// text, suffix array and LCP array resident in HBM (tc_suffix_array_dev, tc_lcp_array_dev: n + 1 entries each)
inline void suffixArrayDev(const uint8_t *d_text, uint64_t n, uint32_t *d_sa) {
    Context::check(tc_suffix_array_dev(Context::get(), d_text, n, d_sa));
}
inline void lcpArrayDev(const uint8_t *d_text, uint64_t n, const uint32_t *d_sa, uint32_t *d_lcp) {
    Context::check(tc_lcp_array_dev(Context::get(), d_text, n, d_sa, d_lcp));
}
struct LCPSummary {
    uint32_t maxLcp;   // the largest entry
    uint64_t row;      // the smallest row holding it: rows row - 1 and row of the suffix array are the longest repeat
    uint64_t sum;      // of all entries: the text has n (n + 1) / 2 - sum distinct substrings
};
inline LCPSummary lcpSummaryDev(const uint32_t *d_lcp, uint64_t N) {
    LCPSummary s{};
    Context::check(tc_lcp_summary_dev(Context::get(), d_lcp, N, &s.maxLcp, &s.row, &s.sum));
    return s;
}
}  // namespace BWT

namespace MTF {
struct MTFB {  // MTF ByteString = (Seq Int, Seq (Maybe ByteString))    (MTF/Internal.hs:67)
    std::vector<int> indices;
    BSSeq finalList;
    bool operator==(const MTFB &o) const { return indices == o.indices && finalList == o.finalList; }
};
// bytestringBWTToMTFB :: BWT Word8 -> MTF ByteString                       (MTF.hs:117-122)
inline MTFB bytestringBWTToMTFB(const Word8Seq &bwt) {
    MTFB out;
    if (bwt.empty()) return out;
    std::vector<int16_t> sym = detail::toSym(bwt);
    std::vector<uint16_t> idx(bwt.size());
    int16_t fl[TC_MAX_SIGMA];
    uint32_t sigma = 0;
    Context::check(tc_mtf_encode_sym(Context::get(), sym.data(), sym.size(), idx.data(), fl, &sigma));
    out.indices.assign(idx.begin(), idx.end());
    for (uint32_t i = 0; i < sigma; i++)
        out.finalList.push_back(fl[i] < 0 ? std::nullopt : std::optional<std::string>(std::string(1, (char)fl[i])));
    return out;
}
// bytestringToBWTToMTFB                                                   (MTF.hs:82-84)
inline MTFB bytestringToBWTToMTFB(const std::string &bs) { return bytestringBWTToMTFB(BWT::bytestringToBWT(bs)); }
// bytestringBWTFromMTFB :: MTF ByteString -> BWT ByteString               (MTF.hs:240-245)
inline Word8Seq bytestringBWTFromMTFB(const MTFB &m) {
    if (m.indices.empty() || m.finalList.empty()) return {};
    std::vector<uint16_t> idx(m.indices.begin(), m.indices.end());
    std::vector<int16_t> fl;
    for (auto &e : m.finalList) fl.push_back(e ? (int16_t)(uint8_t)(*e)[0] : (int16_t)-1);
    std::vector<int16_t> sym(idx.size());
    Context::check(tc_mtf_decode(Context::get(), idx.data(), idx.size(), fl.data(), (uint32_t)fl.size(), sym.data()));
    return detail::fromSym(sym);
}
// bytestringFromBWTFromMTFB                                               (MTF.hs:184-186)
inline std::string bytestringFromBWTFromMTFB(const MTFB &m) { return BWT::bytestringFromWord8BWT(bytestringBWTFromMTFB(m)); }
}  // namespace MTF

namespace RLE {
// bytestringBWTToRLEB :: BWT Word8 -> RLE ByteString                       (RLE.hs:117-123)
inline BSSeq bytestringBWTToRLEB(const Word8Seq &bwt) {
    BSSeq out;
    if (bwt.empty()) return out;  // RLE.hs:119
    std::vector<int16_t> sym = detail::toSym(bwt);
    uint64_t nruns = 2 * bwt.size() + 2;
    std::vector<uint32_t> counts(nruns);
    std::vector<int16_t> syms(nruns);
    Context::check(tc_rle_encode_sym(Context::get(), sym.data(), sym.size(), counts.data(), syms.data(), &nruns));
    for (uint64_t k = 0; k < nruns; k++) {
        out.push_back(std::to_string(counts[k]));  // `show count` (RLE/Internal.hs:128)
        out.push_back(syms[k] < 0 ? std::nullopt : std::optional<std::string>(std::string(1, (char)syms[k])));
    }
    return out;
}
// bytestringToBWTToRLEB                                                   (RLE.hs:83-85)
inline BSSeq bytestringToBWTToRLEB(const std::string &bs) { return bytestringBWTToRLEB(BWT::bytestringToBWT(bs)); }
// bytestringBWTFromRLEB :: RLE ByteString -> BWT ByteString               (RLE.hs:237-241)
inline Word8Seq bytestringBWTFromRLEB(const BSSeq &rle) {
    if (rle.empty()) return {};
    std::vector<uint32_t> counts;
    std::vector<int16_t> syms;
    for (size_t k = 0; k + 1 < rle.size(); k += 2) {  // a trailing odd element is ignored (:187-189)
        const auto &y1 = rle[k], &y2 = rle[k + 1];
        if (y1 && !y2) {
            counts.push_back(1);
            syms.push_back(-1);
            continue;
        }
        if (!y1 || !y2) throw TextCompError(TC_ERR_MALFORMED, "Maybe.fromJust: Nothing (RLE/Internal.hs:172-173)");
        size_t used = 0;
        long long c = 0;
        try {
            c = std::stoll(*y1, &used);
        } catch (...) {
            used = 0;
        }
        if (used != y1->size() || y1->empty()) throw TextCompError(TC_ERR_MALFORMED, "Prelude.read: no parse (RLE/Internal.hs:172)");
        counts.push_back(c > 0 ? (uint32_t)c : 0u);  // replicateM_ of a non-positive count is a no-op
        syms.push_back((int16_t)(uint8_t)(*y2)[0]);
    }
    uint64_t N = 1;
    for (size_t k = 0; k < counts.size(); k++) N += syms[k] < 0 ? 1 : counts[k];
    std::vector<int16_t> out(N);
    if (counts.empty()) return {};
    Context::check(tc_rle_decode(Context::get(), counts.data(), syms.data(), counts.size(), out.data(), &N));
    out.resize(N);
    return detail::fromSym(out);
}
// bytestringFromBWTFromRLEB                                               (RLE.hs:184-186)
inline std::string bytestringFromBWTFromRLEB(const BSSeq &rle) { return BWT::bytestringFromWord8BWT(bytestringBWTFromRLEB(rle)); }
}  // namespace RLE

namespace FMIndex {
using CountResult = std::vector<std::pair<std::string, std::optional<int64_t>>>;
// bytestringFMIndexCountS :: [ByteString] -> ByteString -> Seq (ByteString, Maybe Int)  (FMIndex.hs:362-379)
inline CountResult bytestringFMIndexCountS(const std::vector<std::string> &pats, const std::string &input) {
    CountResult out;
    if (pats.empty() || input.empty()) return out;  // FMIndex.hs:365-366
    tc_fm *fm = nullptr;
    Context::check(tc_fm_build(Context::get(), (const uint8_t *)input.data(), input.size(), &fm));
    std::string flat;
    std::vector<uint64_t> offs(1, 0);
    for (auto &p : pats) {
        flat += p;
        offs.push_back(flat.size());
    }
    flat.push_back('\0');
    std::vector<int64_t> counts(pats.size());
    int rc = tc_fm_count(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), counts.data());
    tc_fm_free(fm);
    Context::check(rc);
    for (size_t i = 0; i < pats.size(); i++)
        out.emplace_back(pats[i], counts[i] ? std::optional<int64_t>(counts[i]) : std::nullopt);
    return out;
}
// bytestringFMIndexCountP (FMIndex.hs:411-432): same values, same order; the spark pool over
// the pattern list is one batched launch.
inline CountResult bytestringFMIndexCountP(const std::vector<std::string> &pats, const std::string &input) {
    return bytestringFMIndexCountS(pats, input);
}

// Not in the reference: search with mismatches -- the text positions within Hamming distance k of each pattern
// (substitutions only, k at most TC_FM_MAX_MISMATCH; a pattern byte that does not occur in the text can only be a
// mismatch; textcomp.h).  The value shapes of the count / locate mirrors: Nothing for no hit.
namespace detail {
inline std::string packPatterns(const std::vector<std::string> &pats, std::vector<uint64_t> &offs) {
    std::string flat;
    offs.assign(1, 0);
    for (auto &p : pats) {
        flat += p;
        offs.push_back(flat.size());
    }
    flat.push_back('\0');
    return flat;
}
}  // namespace detail
inline CountResult bytestringFMIndexCountMismatchS(const std::vector<std::string> &pats, const std::string &input, uint32_t k) {
    CountResult out;
    if (pats.empty() || input.empty()) return out;
    tc_fm *fm = nullptr;
    Context::check(tc_fm_build(Context::get(), (const uint8_t *)input.data(), input.size(), &fm));
    std::vector<uint64_t> offs;
    const std::string flat = detail::packPatterns(pats, offs);
    std::vector<int64_t> counts(pats.size());
    int rc = tc_fm_count_mm(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), k, counts.data());
    tc_fm_free(fm);
    Context::check(rc);
    for (size_t i = 0; i < pats.size(); i++)
        out.emplace_back(pats[i], counts[i] ? std::optional<int64_t>(counts[i]) : std::nullopt);
    return out;
}
inline CountResult bytestringFMIndexCountMismatchP(const std::vector<std::string> &pats, const std::string &input, uint32_t k) {
    return bytestringFMIndexCountMismatchS(pats, input, k);
}
// per pattern: (1-based position, mismatches) of every hit, each once, in the device's enumeration order (deterministic, not
// sorted)
using LocateMismatchResult = std::vector<std::pair<std::string, std::vector<std::pair<uint64_t, uint8_t>>>>;
inline LocateMismatchResult bytestringFMIndexLocateMismatchS(const std::vector<std::string> &pats, const std::string &input,
                                                             uint32_t k) {
    LocateMismatchResult out;
    if (pats.empty() || input.empty()) return out;
    tc_fm *fm = nullptr;
    Context::check(tc_fm_build(Context::get(), (const uint8_t *)input.data(), input.size(), &fm));
    std::vector<uint64_t> offs;
    const std::string flat = detail::packPatterns(pats, offs);
    std::vector<uint64_t> hoffs(pats.size() + 1), hits(16 * pats.size());
    std::vector<uint8_t> mm(hits.size());
    uint64_t nh = hits.size();
    int rc = tc_fm_locate_mm(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), k, hoffs.data(),
                             hits.data(), mm.data(), &nh);
    if (rc == TC_ERR_CAPACITY) {            // *nhits = the hits needed: once more with room for them
        hits.resize(nh);
        mm.resize(nh);
        rc = tc_fm_locate_mm(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), k, hoffs.data(),
                             hits.data(), mm.data(), &nh);
    }
    tc_fm_free(fm);
    Context::check(rc);
    for (size_t i = 0; i < pats.size(); i++) {
        std::vector<std::pair<uint64_t, uint8_t>> h;
        for (uint64_t t = hoffs[i]; t < hoffs[i + 1]; t++) h.emplace_back(hits[t], mm[t]);
        out.emplace_back(pats[i], std::move(h));
    }
    return out;
}
inline LocateMismatchResult bytestringFMIndexLocateMismatchP(const std::vector<std::string> &pats, const std::string &input,
                                                             uint32_t k) {
    return bytestringFMIndexLocateMismatchS(pats, input, k);
}

// Not in the reference: factorize -- the greedy right-to-left longest-match parse of each pattern against the text
// (textcomp.h).  Per pattern its factors in pattern order, in the ABI's convention: a match is (1-based text position of the
// occurrence in the first suffix-array row, length >= 1), a literal -- a byte the text does not hold -- is (byte value, 0).
// An empty pattern list gives an empty result; against an empty text every byte is a literal.
struct Factors {
    std::vector<uint64_t> offs, pos;    // offs [npat + 1]: pattern i's factors are [offs[i], offs[i + 1])
    std::vector<uint32_t> len;
};
namespace detail {
inline Factors factorize(const tc_fm *fm, const std::vector<std::string> &pats) {
    Factors f;
    f.offs.assign(pats.size() + 1, 0);
    if (pats.empty()) return f;
    std::vector<uint64_t> offs;
    const std::string flat = packPatterns(pats, offs);
    uint64_t nf = 0;        // the sizes-only form first: the total
    Context::check(tc_fm_factorize(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), f.offs.data(),
                                   nullptr, nullptr, &nf));
    f.pos.resize(nf);
    f.len.resize(nf);
    if (nf)
        Context::check(tc_fm_factorize(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), f.offs.data(),
                                       f.pos.data(), f.len.data(), &nf));
    return f;
}
}  // namespace detail
using FactorizeResult = std::vector<std::pair<std::string, std::vector<std::pair<uint64_t, uint32_t>>>>;
inline FactorizeResult bytestringFMIndexFactorizeS(const std::vector<std::string> &pats, const std::string &input) {
    FactorizeResult out;
    if (pats.empty()) return out;
    tc_fm *fm = nullptr;
    Context::check(tc_fm_build(Context::get(), (const uint8_t *)input.data(), input.size(), &fm));
    Factors f;
    try {
        f = detail::factorize(fm, pats);
    } catch (...) {
        tc_fm_free(fm);
        throw;
    }
    tc_fm_free(fm);
    for (size_t i = 0; i < pats.size(); i++) {
        std::vector<std::pair<uint64_t, uint32_t>> v;
        for (uint64_t t = f.offs[i]; t < f.offs[i + 1]; t++) v.emplace_back(f.pos[t], f.len[t]);
        out.emplace_back(pats[i], std::move(v));
    }
    return out;
}
inline FactorizeResult bytestringFMIndexFactorizeP(const std::vector<std::string> &pats, const std::string &input) {
    return bytestringFMIndexFactorizeS(pats, input);
}

// Not in the reference: matching statistics and maximal exact matches (textcomp.h).  For every position i of every pattern
// the length of the longest match that starts there, the 1-based text position of its occurrence in the first
// suffix-array row and the number of its occurrences -- (0, 0, 0) where the byte does not occur -- flat, pattern after
// pattern (pattern j's entries are [offs[j], offs[j + 1])); the MEMs are the matches of at least min_len bytes that are
// contained in no longer match of the same pattern, per pattern in increasing start.  The index must hold the LCP part.
struct MatchStats {
    std::vector<uint64_t> offs, pos;    // offs [npat + 1]: the pattern offsets
    std::vector<uint32_t> len, occ;
};
struct Mems {
    std::vector<uint64_t> offs, start, pos;     // offs [npat + 1]: pattern i's MEMs are [offs[i], offs[i + 1])
    std::vector<uint32_t> len;
};
namespace detail {
inline MatchStats matchStats(const tc_fm *fm, const std::vector<std::string> &pats) {
    MatchStats r;
    r.offs.assign(pats.size() + 1, 0);
    if (pats.empty()) return r;
    const std::string flat = packPatterns(pats, r.offs);
    const uint64_t total = r.offs.back();
    r.pos.assign(total + 1, 0);
    r.len.assign(total + 1, 0);
    r.occ.assign(total + 1, 0);
    Context::check(tc_fm_match_stats(Context::get(), fm, (const uint8_t *)flat.data(), r.offs.data(), pats.size(), r.len.data(),
                                     r.pos.data(), r.occ.data()));
    r.pos.resize(total);
    r.len.resize(total);
    r.occ.resize(total);
    return r;
}
inline Mems mems(const tc_fm *fm, const std::vector<std::string> &pats, uint32_t min_len) {
    Mems r;
    r.offs.assign(pats.size() + 1, 0);
    if (pats.empty()) return r;
    std::vector<uint64_t> offs;
    const std::string flat = packPatterns(pats, offs);
    uint64_t nm = 0;        // the sizes-only form first: the total
    Context::check(tc_fm_mems(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), min_len, r.offs.data(),
                              nullptr, nullptr, nullptr, &nm));
    r.start.resize(nm);
    r.pos.resize(nm);
    r.len.resize(nm);
    if (nm)
        Context::check(tc_fm_mems(Context::get(), fm, (const uint8_t *)flat.data(), offs.data(), pats.size(), min_len,
                                  r.offs.data(), r.start.data(), r.pos.data(), r.len.data(), &nm));
    return r;
}
}  // namespace detail
// per pattern its (len, pos, occ) triples, one per position
using MatchStatsResult = std::vector<std::pair<std::string, std::vector<std::array<uint64_t, 3>>>>;
inline MatchStatsResult bytestringFMIndexMatchStatsS(const std::vector<std::string> &pats, const std::string &input) {
    MatchStatsResult out;
    if (pats.empty()) return out;
    tc_fm *fm = nullptr;
    Context::check(tc_fm_build_lcp(Context::get(), (const uint8_t *)input.data(), input.size(), 1, 0, &fm));
    MatchStats r;
    try {
        r = detail::matchStats(fm, pats);
    } catch (...) {
        tc_fm_free(fm);
        throw;
    }
    tc_fm_free(fm);
    for (size_t i = 0; i < pats.size(); i++) {
        std::vector<std::array<uint64_t, 3>> v;
        for (uint64_t t = r.offs[i]; t < r.offs[i + 1]; t++) v.push_back({(uint64_t)r.len[t], r.pos[t], (uint64_t)r.occ[t]});
        out.emplace_back(pats[i], std::move(v));
    }
    return out;
}
inline MatchStatsResult bytestringFMIndexMatchStatsP(const std::vector<std::string> &pats, const std::string &input) {
    return bytestringFMIndexMatchStatsS(pats, input);
}
// per pattern its (start, pos, len) triples, start 0-based in the pattern
using MemsResult = std::vector<std::pair<std::string, std::vector<std::array<uint64_t, 3>>>>;
inline MemsResult bytestringFMIndexMemsS(const std::vector<std::string> &pats, const std::string &input, uint32_t min_len = 1) {
    MemsResult out;
    if (pats.empty()) return out;
    tc_fm *fm = nullptr;
    Context::check(tc_fm_build_lcp(Context::get(), (const uint8_t *)input.data(), input.size(), 1, 0, &fm));
    Mems r;
    try {
        r = detail::mems(fm, pats, min_len);
    } catch (...) {
        tc_fm_free(fm);
        throw;
    }
    tc_fm_free(fm);
    for (size_t i = 0; i < pats.size(); i++) {
        std::vector<std::array<uint64_t, 3>> v;
        for (uint64_t t = r.offs[i]; t < r.offs[i + 1]; t++) v.push_back({r.start[t], r.pos[t], (uint64_t)r.len[t]});
        out.emplace_back(pats[i], std::move(v));
    }
    return out;
}
inline MemsResult bytestringFMIndexMemsP(const std::vector<std::string> &pats, const std::string &input, uint32_t min_len = 1) {
    return bytestringFMIndexMemsS(pats, input, min_len);
}

// Not in the reference: an index that is kept between queries, optionally with a sampled suffix array (sa_rate > 1: every
// sa_rate-th entry is kept and locate walks the LF mapping to the next one; textcomp.h), queried with everything in HBM.
class Index {
  public:
    // text in host memory / text already on the device
    Index(const std::string &text, uint32_t sa_rate = 1) {
        Context::check(tc_fm_build_sampled(Context::get(), (const uint8_t *)text.data(), text.size(), sa_rate, &fm_));
    }
    Index(const uint8_t *d_text, uint64_t n, uint32_t sa_rate) {
        Context::check(tc_fm_build_sampled_dev(Context::get(), d_text, n, sa_rate, &fm_));
    }
    // with text samples (text_rate: a power of two >= 1): the index can read text ranges back (extract / extractDev)
    Index(const std::string &text, uint32_t sa_rate, uint32_t text_rate) {
        Context::check(tc_fm_build_self(Context::get(), (const uint8_t *)text.data(), text.size(), sa_rate, text_rate, &fm_));
    }
    Index(const uint8_t *d_text, uint64_t n, uint32_t sa_rate, uint32_t text_rate) {
        Context::check(tc_fm_build_self_dev(Context::get(), d_text, n, sa_rate, text_rate, &fm_));
    }
    // with the LCP part (text_rate: 0 or a power of two): the index answers matchStats / mems
    struct WithLcp {};
    Index(const std::string &text, uint32_t sa_rate, uint32_t text_rate, WithLcp) {
        Context::check(tc_fm_build_lcp(Context::get(), (const uint8_t *)text.data(), text.size(), sa_rate, text_rate, &fm_));
    }
    Index(const uint8_t *d_text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, WithLcp) {
        Context::check(tc_fm_build_lcp_dev(Context::get(), d_text, n, sa_rate, text_rate, &fm_));
    }
    Index(const Index &) = delete;
    Index &operator=(const Index &) = delete;
    ~Index() { tc_fm_free(fm_); }
    uint32_t saRate() const { return tc_fm_sa_rate(fm_); }
    uint32_t textRate() const { return tc_fm_text_rate(fm_); }
    bool hasLcp() const { return tc_fm_has_lcp(fm_) != 0; }
    // part 0: the whole index, part 1: its locate part alone, part 2: its extract part alone, part 3: its LCP part alone
    uint64_t deviceBytes(int part = 0) const { return tc_fm_device_bytes(fm_, part); }
    // d_pats / d_offs [npat + 1] / d_hit_offs [npat + 1] / d_hits [cap]: device arrays.  Returns the number of hits; when it
    // exceeds cap nothing was written to d_hits and the caller repeats the call with that capacity.
    uint64_t locateDev(const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint64_t *d_hit_offs, uint64_t *d_hits,
                       uint64_t cap) const {
        uint64_t nh = cap;
        int rc = tc_fm_locate_dev(Context::get(), fm_, d_pats, d_offs, npat, d_hit_offs, d_hits, &nh);
        if (rc != TC_ERR_CAPACITY) Context::check(rc);
        return nh;
    }
    // the text ranges [starts[q], starts[q] + lens[q]), starts 1-based as locate answers positions; one string per query
    std::vector<std::string> extract(const std::vector<uint64_t> &starts, const std::vector<uint64_t> &lens) const {
        std::vector<std::string> res(starts.size());
        if (starts.empty() || lens.size() != starts.size()) return res;
        uint64_t total = 0;
        for (uint64_t l : lens) total += l;
        std::vector<uint64_t> offs(starts.size() + 1);
        std::string flat(total, '\0');
        uint64_t nb = total;
        Context::check(tc_fm_extract(Context::get(), fm_, starts.data(), lens.data(), starts.size(), offs.data(),
                                     (uint8_t *)&flat[0], &nb));
        for (size_t q = 0; q < starts.size(); q++) res[q] = flat.substr(offs[q], offs[q + 1] - offs[q]);
        return res;
    }
    // d_starts / d_lens [nq] / d_out_offs [nq + 1] / d_out [cap]: device arrays.  Returns the number of bytes; when it
    // exceeds cap nothing was written to d_out and the caller repeats the call with that capacity.
    uint64_t extractDev(const uint64_t *d_starts, const uint64_t *d_lens, uint64_t nq, uint64_t *d_out_offs, uint8_t *d_out,
                        uint64_t cap) const {
        uint64_t nb = cap;
        int rc = tc_fm_extract_dev(Context::get(), fm_, d_starts, d_lens, nq, d_out_offs, d_out, &nb);
        if (rc != TC_ERR_CAPACITY) Context::check(rc);
        return nb;
    }
    // the factors of every pattern (bytestringFMIndexFactorizeS on the kept index), and their inverse on an index with text
    // samples: unfactorize(factorize(pats)) == pats, and the text itself need not be kept
    Factors factorize(const std::vector<std::string> &pats) const { return detail::factorize(fm_, pats); }
    std::vector<std::string> unfactorize(const Factors &f) const {
        const size_t npat = f.offs.empty() ? 0 : f.offs.size() - 1;
        std::vector<std::string> res(npat);
        if (!npat) return res;
        std::vector<uint64_t> offs(npat + 1);
        std::string flat(1, '\0');
        uint64_t nb = 0;
        int rc = tc_fm_unfactorize(Context::get(), fm_, f.offs.data(), f.pos.data(), f.len.data(), npat, offs.data(),
                                   (uint8_t *)&flat[0], &nb);
        if (rc == TC_ERR_CAPACITY) {            // *nbytes = the bytes needed: once more with room for them
            flat.assign(nb, '\0');
            rc = tc_fm_unfactorize(Context::get(), fm_, f.offs.data(), f.pos.data(), f.len.data(), npat, offs.data(),
                                   (uint8_t *)&flat[0], &nb);
        }
        Context::check(rc);
        for (size_t i = 0; i < npat; i++) res[i] = flat.substr(offs[i], offs[i + 1] - offs[i]);
        return res;
    }
    // everything in HBM (d_fac_offs [npat + 1], d_fac_pos / d_fac_len [cap]; d_out_offs [npat + 1], d_out [cap]).  Each returns
    // the total; when it exceeds cap nothing was written to the payload arrays and the caller repeats the call with it.
    uint64_t factorizeDev(const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint64_t *d_fac_offs, uint64_t *d_fac_pos,
                          uint32_t *d_fac_len, uint64_t cap) const {
        uint64_t nf = cap;
        int rc = tc_fm_factorize_dev(Context::get(), fm_, d_pats, d_offs, npat, d_fac_offs, d_fac_pos, d_fac_len, &nf);
        if (rc != TC_ERR_CAPACITY) Context::check(rc);
        return nf;
    }
    uint64_t unfactorizeDev(const uint64_t *d_fac_offs, const uint64_t *d_fac_pos, const uint32_t *d_fac_len, uint64_t npat,
                            uint64_t *d_out_offs, uint8_t *d_out, uint64_t cap) const {
        uint64_t nb = cap;
        int rc = tc_fm_unfactorize_dev(Context::get(), fm_, d_fac_offs, d_fac_pos, d_fac_len, npat, d_out_offs, d_out, &nb);
        if (rc != TC_ERR_CAPACITY) Context::check(rc);
        return nb;
    }
    // matching statistics and maximal exact matches on an index with the LCP part (bytestringFMIndexMatchStatsS / ...MemsS
    // on the kept index), and the same with everything in HBM: d_ms_len [offs[npat]] and, each or null, d_ms_pos / d_ms_occ;
    // d_mem_offs [npat + 1], d_mem_start / d_mem_pos / d_mem_len [cap] -- memsDev returns the total; when it exceeds cap
    // nothing was written to the three arrays and the caller repeats the call with it
    MatchStats matchStats(const std::vector<std::string> &pats) const { return detail::matchStats(fm_, pats); }
    Mems mems(const std::vector<std::string> &pats, uint32_t min_len = 1) const { return detail::mems(fm_, pats, min_len); }
    void matchStatsDev(const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t *d_ms_len, uint64_t *d_ms_pos,
                       uint32_t *d_ms_occ) const {
        Context::check(tc_fm_match_stats_dev(Context::get(), fm_, d_pats, d_offs, npat, d_ms_len, d_ms_pos, d_ms_occ));
    }
    uint64_t memsDev(const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t min_len, uint64_t *d_mem_offs,
                     uint64_t *d_mem_start, uint64_t *d_mem_pos, uint32_t *d_mem_len, uint64_t cap) const {
        uint64_t nm = cap;
        int rc = tc_fm_mems_dev(Context::get(), fm_, d_pats, d_offs, npat, min_len, d_mem_offs, d_mem_start, d_mem_pos, d_mem_len,
                                &nm);
        if (rc != TC_ERR_CAPACITY) Context::check(rc);
        return nm;
    }
    const tc_fm *handle() const { return fm_; }

  private:
    tc_fm *fm_ = nullptr;
};
}  // namespace FMIndex

}  // namespace Data
