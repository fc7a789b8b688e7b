// What the stand-alone host checks of this directory share and need nothing of csrc/ for: EXPECT, heap blocks of exact size,
// the enhanced suffix array of a text built naively, and the texts.  A check includes this header (or check_esa.hpp, which
// includes it) after its kernel header.
//
// The blocks are the point of these programs: a kernel body reads and writes arrays that hold exactly the entries the check
// decides, so the sanitizer stops the run at an access one element outside.  Nothing here rounds a size up or shares a block
// between two arrays, and what the builders below return are std::vectors: a check copies them into blocks of the sizes it
// chooses (block_of, or block / block_bytes and a copy) before a kernel sees them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// ---- heap blocks of exactly the entries asked for (one entry where none is asked for) -------------------------------------
template <class T>
static std::unique_ptr<T[]> block(size_t count) { return std::unique_ptr<T[]>(new T[count ? count : 1]); }
template <class T>
static std::unique_ptr<T[]> block(size_t count, T fill) {
    auto p = block<T>(count);
    std::fill(p.get(), p.get() + count, fill);
    return p;
}
template <class T>
static std::unique_ptr<T[]> block_of(const std::vector<T> &v) {
    auto p = block<T>(v.size());
    std::copy(v.begin(), v.end(), p.get());
    return p;
}
// a block of exactly `bytes` bytes, for the arrays whose size the library states in bytes
template <class T>
static std::unique_ptr<T[]> block_bytes(size_t bytes) {
    EXPECT(bytes % sizeof(T) == 0);
    return block<T>(bytes / sizeof(T));
}

// ---- the enhanced suffix array of a text, naively: N = n + 1 rows --------------------------------------------------------
// the suffixes in order, the empty one first: a proper prefix sorts first
static std::vector<uint32_t> sort_suffixes(const Bytes &t) {
    const uint32_t n = (uint32_t)t.size();
    std::vector<uint32_t> sa(n + 1);
    for (uint32_t i = 0; i <= n; i++) sa[i] = i;
    std::sort(sa.begin(), sa.end(), [&](uint32_t x, uint32_t y) {
        const int c = std::memcmp(t.data() + x, t.data() + y, std::min(n - x, n - y));
        return c ? c < 0 : x > y;
    });
    return sa;
}
// lcp[j] = the common prefix of the suffixes of rows j - 1 and j, by comparing them; lcp[0] = 0
static std::vector<uint32_t> lcp_of(const Bytes &t, const std::vector<uint32_t> &sa) {
    const uint32_t n = (uint32_t)t.size();
    std::vector<uint32_t> lcp(sa.size(), 0);
    for (size_t j = 1; j < sa.size(); j++) {
        const uint32_t a = sa[j - 1], b = sa[j];
        uint32_t l = 0;
        while (a + l < n && b + l < n && t[a + l] == t[b + l]) l++;
        lcp[j] = l;
    }
    return lcp;
}
// isa[sa[j]] = j
static std::vector<uint32_t> inverse_of(const std::vector<uint32_t> &sa) {
    std::vector<uint32_t> isa(sa.size());
    for (size_t j = 0; j < sa.size(); j++) isa[sa[j]] = (uint32_t)j;
    return isa;
}

// ---- texts -----------------------------------------------------------------------------------------------------------------
// alphabets: the first `count` bytes of `s`; `count` byte values from `first` on, `step` apart (modulo 256)
static Bytes letters(const char *s, size_t count) { return Bytes(s, s + count); }
static Bytes byte_values(uint32_t first, uint32_t count, uint32_t step = 1) {
    Bytes al(count);
    for (uint32_t i = 0; i < count; i++) al[i] = (uint8_t)(first + i * step);
    return al;
}
// n bytes drawn from an alphabet, one draw of the generator per byte
template <class Rng>
static Bytes random_text(Rng &rng, size_t n, const Bytes &alphabet) {
    Bytes t(n);
    for (uint8_t &b : t) b = alphabet[rng() % alphabet.size()];
    return t;
}
// the same by the alphabet's size: up to 4 the first letters of ACGT, 256 every byte value, otherwise the codes 1 .. sigma
static Bytes random_text(std::mt19937 &rng, size_t n, uint32_t sigma) {
    return random_text(rng, n, sigma <= 4 ? letters("ACGT", sigma) : sigma == 256 ? byte_values(0, 256) : byte_values(1, sigma));
}
// period p <= 7, starting `phase` bytes into the period
static Bytes periodic(uint32_t n, uint32_t p, uint32_t phase = 0, const char *period = "ACGTNXY") {
    Bytes t(n);
    for (uint32_t i = 0; i < n; i++) t[i] = (uint8_t)period[(i + phase) % p];
    return t;
}
// the first n bytes of the Fibonacci word a ab aba abaab ...
static Bytes fibonacci(uint32_t n, char first = 'A', char second = 'B') {
    std::string a(1, first), b = a + second;
    while (b.size() < n) {
        const std::string c = b + a;
        a = b;
        b = c;
    }
    return Bytes(b.begin(), b.begin() + n);
}
