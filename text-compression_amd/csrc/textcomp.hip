// textcomp.hip -- libtextcomp.so: the C ABI (include/textcomp.h) over the HIP kernels: the context, the bounds, what
// reads a header in host memory, and one forwarding wrapper per entry point (the bodies: the *_entry functions of the
// csrc/ headers).  Single translation unit for gfx950: hipcc --offload-arch=gfx950 -shared -fPIC.
#include "tc_common.hpp"
#include "tc_encode_host.hpp"
#include "tc_decode_host.hpp"
#include "tc_ws_host.hpp"
#include "tc_fm_host.hpp"
#include "tc_lcp_host.hpp"
#include "tc_esa_plan.hpp"
#include "tc_lz_host.hpp"
#include "tc_rep_host.hpp"
#include "tc_kmer_host.hpp"
#include "tc_tm_host.hpp"
#include "tc_tr_host.hpp"
#include "tc_pal_host.hpp"
#include "tc_maw_host.hpp"
#include "tc_sus_host.hpp"
#include "tc_cov_host.hpp"
#include "tc_esa_host.hpp"
#include "tc_esa_docs_host.hpp"
#include "tc_esa_xdoc_host.hpp"
#include "tc_container_host.hpp"
#include "tc_hostio_host.hpp"
#include "tc_generate.hpp"
#include "tc_dbg_host.hpp"
#include "tc_comm.hpp"
#include "textcomp_debug.h"

#define TC_API_BEGIN(ctx)                                  \
    if (!(ctx)) return TC_ERR_ARG;                         \
    try {                                                  \
        if (hipSetDevice((ctx)->device) != hipSuccess) {   \
            (ctx)->err = "hipSetDevice failed";            \
            return TC_ERR_HIP;                             \
        }
#define TC_API_END(ctx)                                    \
        return TC_OK;                                      \
    } catch (const TcFail &f) {                            \
        (void)hipGetLastError();                           \
        return f.code;                                     \
    } catch (...) {                                        \
        (ctx)->err = "unexpected exception";               \
        return TC_ERR_INTERNAL;                            \
    }

extern "C" {

const char *tc_version(void) { return "textcomp-amd 0.1 (gfx950)"; }

int tc_ctx_create(int device, tc_ctx **out) {
    if (!out) return TC_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return TC_ERR_HIP;  // no CPU fallback, by design
    }
    if (device < 0 || device >= count) return TC_ERR_ARG;
    tc_ctx *ctx = new tc_ctx();
    ctx->device = device;
    try {
        TC_HIP(ctx, hipSetDevice(device));
        {
            hipDeviceProp_t prop;
            TC_HIP(ctx, hipGetDeviceProperties(&prop, device));
            ctx->num_cus = prop.multiProcessorCount;
        }
        TC_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        TC_HIP(ctx, hipMalloc((void **)&ctx->d_err, 256));
        TC_HIP(ctx, hipMalloc((void **)&ctx->d_scalars, 128 * sizeof(u64)));
        TC_HIP(ctx, hipHostMalloc((void **)&ctx->h_scalars, 64 * sizeof(u64), hipHostMallocDefault));
        TC_HIP(ctx, hipHostMalloc((void **)&ctx->h_hdr, 1024, hipHostMallocDefault));
        TC_HIP(ctx, hipMemsetAsync(ctx->d_err, 0, 256, ctx->stream));
        TC_HIP(ctx, hipMemsetAsync(ctx->d_scalars, 0, 128 * sizeof(u64), ctx->stream));
        for (int i = 0; i < 8; i++) TC_HIP(ctx, hipEventCreate(&ctx->ev[i]));
        for (int i = 0; i < 32; i++) TC_HIP(ctx, hipEventCreate(&ctx->pev[i]));
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } catch (const TcFail &f) {
        int code = f.code;
        tc_ctx_destroy(ctx);
        return code;
    }
    *out = ctx;
    return TC_OK;
}

void tc_ctx_destroy(tc_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 8; i++)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    for (int i = 0; i < 32; i++)
        if (ctx->pev[i]) (void)hipEventDestroy(ctx->pev[i]);
    hp_release(ctx);
    tc_ws_release(ctx);
    if (ctx->d_err) (void)hipFree(ctx->d_err);
    if (ctx->d_scalars) (void)hipFree(ctx->d_scalars);
    if (ctx->h_scalars) (void)hipHostFree(ctx->h_scalars);
    if (ctx->h_hdr) (void)hipHostFree(ctx->h_hdr);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *tc_last_error(const tc_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int tc_get_stats(const tc_ctx *ctx, tc_stats *out) {
    if (!ctx || !out) return TC_ERR_ARG;
    *out = ctx->stats;
    out->ws_chunks = (uint32_t)ctx->ws_chunks.size();
    out->ws_grown = ctx->stats_ws_grown;
    return TC_OK;
}

void *tc_ctx_stream(const tc_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int tc_ctx_place_workspace(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_block *out, int tries, double *ms,
                           int *chosen) {
    TC_API_BEGIN(ctx)
    ws_place_entry(ctx, d_text, n, out, tries, ms, chosen);
    TC_API_END(ctx)
}

int tc_ctx_set_profile(tc_ctx *ctx, int on) {
    if (!ctx) return TC_ERR_ARG;
    ctx->profile = on ? 1 : 0;
    return TC_OK;
}

int tc_ctx_set_container_coding(tc_ctx *ctx, int coding) {
    if (!ctx) return TC_ERR_ARG;
    if (coding != TC_CODING_PACKED && coding != TC_CODING_HUFFMAN) {
        ctx->err = "unknown container coding";
        return TC_ERR_ARG;
    }
    ctx->coding = coding;
    return TC_OK;
}

int tc_ctx_get_container_coding(const tc_ctx *ctx) { return ctx ? ctx->coding : TC_ERR_ARG; }

// ================================================================= Data.BWT
int tc_bwt_encode_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint8_t *d_L,
                      uint64_t *primary) {
    TC_API_BEGIN(ctx)
    bwt_encode_entry(ctx, d_text, n, d_L, primary, true);
    TC_API_END(ctx)
}

int tc_bwt_encode(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *L, uint64_t *primary) {
    TC_API_BEGIN(ctx)
    bwt_encode_entry(ctx, text, n, L, primary, false);
    TC_API_END(ctx)
}

int tc_suffix_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sa) {
    TC_API_BEGIN(ctx)
    suffix_array_entry(ctx, text, n, sa);
    TC_API_END(ctx)
}

// the enhanced suffix array (an addition to the reference's surface): tc_lcp_host.hpp
int tc_suffix_array_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_sa) {
    TC_API_BEGIN(ctx)
    suffix_array_dev_entry(ctx, d_text, n, d_sa);
    TC_API_END(ctx)
}

int tc_lcp_array_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint32_t *d_sa, uint32_t *d_lcp) {
    TC_API_BEGIN(ctx)
    lcp_array_dev_entry(ctx, d_text, n, d_sa, d_lcp);
    TC_API_END(ctx)
}

int tc_lcp_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sa, uint32_t *lcp) {
    TC_API_BEGIN(ctx)
    lcp_array_host_entry(ctx, text, n, sa, lcp);
    TC_API_END(ctx)
}

int tc_lcp_summary_dev(tc_ctx *ctx, const uint32_t *d_lcp, uint64_t N, uint32_t *max_lcp, uint64_t *row, uint64_t *sum) {
    TC_API_BEGIN(ctx)
    lcp_summary_entry(ctx, d_lcp, N, max_lcp, row, sum);
    TC_API_END(ctx)
}

// the LPF array, the LZ77 parse of a text against itself and its inverse (no counterpart in the reference): tc_lz_host.hpp
int tc_lpf_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *lpf, uint32_t *src) {
    TC_API_BEGIN(ctx)
    lpf_array_entry(ctx, text, n, lpf, src, false);
    TC_API_END(ctx)
}

int tc_lpf_array_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_lpf, uint32_t *d_src) {
    TC_API_BEGIN(ctx)
    lpf_array_entry(ctx, d_text, n, d_lpf, d_src, true);
    TC_API_END(ctx)
}

int tc_lz_parse(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *ph_src, uint32_t *ph_len, uint64_t *nph) {
    TC_API_BEGIN(ctx)
    lz_parse_entry(ctx, text, n, ph_src, ph_len, nph, false);
    TC_API_END(ctx)
}

int tc_lz_parse_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_ph_src, uint32_t *d_ph_len, uint64_t *nph) {
    TC_API_BEGIN(ctx)
    lz_parse_entry(ctx, d_text, n, d_ph_src, d_ph_len, nph, true);
    TC_API_END(ctx)
}

int tc_lz_unparse(tc_ctx *ctx, const uint32_t *ph_src, const uint32_t *ph_len, uint64_t nph, uint8_t *text, uint64_t *nbytes) {
    TC_API_BEGIN(ctx)
    lz_unparse_entry(ctx, ph_src, ph_len, nph, text, nbytes, false);
    TC_API_END(ctx)
}

int tc_lz_unparse_dev(tc_ctx *ctx, const uint32_t *d_ph_src, const uint32_t *d_ph_len, uint64_t nph, uint8_t *d_text,
                      uint64_t *nbytes) {
    TC_API_BEGIN(ctx)
    lz_unparse_entry(ctx, d_ph_src, d_ph_len, nph, d_text, nbytes, true);
    TC_API_END(ctx)
}

// the maximal and supermaximal repeats of a text (no counterpart in the reference): tc_rep_host.hpp
int tc_repeats(tc_ctx *ctx, const uint8_t *text, uint64_t n, int kind, uint32_t min_len, uint32_t min_occ, uint32_t *sa,
               uint32_t *rep_pos, uint32_t *rep_len, uint32_t *rep_occ, uint32_t *rep_row, uint64_t *nrep) {
    TC_API_BEGIN(ctx)
    repeats_entry(ctx, text, n, kind, min_len, min_occ, sa, rep_pos, rep_len, rep_occ, rep_row, nrep, false);
    TC_API_END(ctx)
}

int tc_repeats_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, int kind, uint32_t min_len, uint32_t min_occ, uint32_t *d_sa,
                   uint32_t *d_rep_pos, uint32_t *d_rep_len, uint32_t *d_rep_occ, uint32_t *d_rep_row, uint64_t *nrep) {
    TC_API_BEGIN(ctx)
    repeats_entry(ctx, d_text, n, kind, min_len, min_occ, d_sa, d_rep_pos, d_rep_len, d_rep_occ, d_rep_row, nrep, true);
    TC_API_END(ctx)
}

// the runs (tandem repeats) of a text (no counterpart in the reference): tc_tr_host.hpp
int tc_tandem_repeats(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_period, uint32_t max_period, uint32_t min_copies,
                      uint32_t min_len, uint32_t *run_start, uint32_t *run_len, uint32_t *run_period, uint64_t *nrun) {
    TC_API_BEGIN(ctx)
    tandem_repeats_entry(ctx, text, n, min_period, max_period, min_copies, min_len, run_start, run_len, run_period, nrun, false);
    TC_API_END(ctx)
}

int tc_tandem_repeats_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_period, uint32_t max_period,
                          uint32_t min_copies, uint32_t min_len, uint32_t *d_run_start, uint32_t *d_run_len, uint32_t *d_run_period,
                          uint64_t *nrun) {
    TC_API_BEGIN(ctx)
    tandem_repeats_entry(ctx, d_text, n, min_period, max_period, min_copies, min_len, d_run_start, d_run_len, d_run_period, nrun, true);
    TC_API_END(ctx)
}

// the palindromes and inverted repeats of a text, with mismatches (no counterpart in the reference): tc_pal_host.hpp
int tc_palindromes(tc_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch, uint32_t min_len,
                   uint32_t *pal_start, uint32_t *pal_len, uint32_t *pal_mm, uint64_t *npal) {
    TC_API_BEGIN(ctx)
    palindromes_entry(ctx, text, n, comp, max_mismatch, min_len, pal_start, pal_len, pal_mm, npal, false);
    TC_API_END(ctx)
}

int tc_palindromes_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch, uint32_t min_len,
                       uint32_t *d_pal_start, uint32_t *d_pal_len, uint32_t *d_pal_mm, uint64_t *npal) {
    TC_API_BEGIN(ctx)
    palindromes_entry(ctx, d_text, n, comp, max_mismatch, min_len, d_pal_start, d_pal_len, d_pal_mm, npal, true);
    TC_API_END(ctx)
}

// the minimal absent words of a text (no counterpart in the reference): tc_maw_host.hpp
int tc_absent_words(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t max_len, uint8_t *maw_left,
                    uint32_t *maw_pos, uint32_t *maw_len, uint64_t *nmaw) {
    TC_API_BEGIN(ctx)
    absent_words_entry(ctx, text, n, min_len, max_len, maw_left, maw_pos, maw_len, nmaw, false);
    TC_API_END(ctx)
}

int tc_absent_words_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t max_len, uint8_t *d_maw_left,
                        uint32_t *d_maw_pos, uint32_t *d_maw_len, uint64_t *nmaw) {
    TC_API_BEGIN(ctx)
    absent_words_entry(ctx, d_text, n, min_len, max_len, d_maw_left, d_maw_pos, d_maw_len, nmaw, true);
    TC_API_END(ctx)
}

int tc_absent_word_profile(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t kmax, uint64_t *hist, uint64_t *total) {
    TC_API_BEGIN(ctx)
    absent_word_profile_entry(ctx, text, n, kmax, hist, total, false);
    TC_API_END(ctx)
}

int tc_absent_word_profile_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t kmax, uint64_t *d_hist, uint64_t *total) {
    TC_API_BEGIN(ctx)
    absent_word_profile_entry(ctx, d_text, n, kmax, d_hist, total, true);
    TC_API_END(ctx)
}

// what is unique in a text: shortest unique prefixes, minimal unique substrings, the shortest unique substring over every
// position (no counterpart in the reference): tc_sus_host.hpp
int tc_unique_prefixes(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *up) {
    TC_API_BEGIN(ctx)
    unique_prefixes_entry(ctx, text, n, up, false);
    TC_API_END(ctx)
}

int tc_unique_prefixes_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_up) {
    TC_API_BEGIN(ctx)
    unique_prefixes_entry(ctx, d_text, n, d_up, true);
    TC_API_END(ctx)
}

int tc_unique_substrings(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t max_len, uint32_t *mus_start,
                         uint32_t *mus_len, uint64_t *nmus) {
    TC_API_BEGIN(ctx)
    unique_substrings_entry(ctx, text, n, min_len, max_len, mus_start, mus_len, nmus, false);
    TC_API_END(ctx)
}

int tc_unique_substrings_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t max_len, uint32_t *d_mus_start,
                             uint32_t *d_mus_len, uint64_t *nmus) {
    TC_API_BEGIN(ctx)
    unique_substrings_entry(ctx, d_text, n, min_len, max_len, d_mus_start, d_mus_len, nmus, true);
    TC_API_END(ctx)
}

int tc_shortest_unique(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sus_start, uint32_t *sus_len) {
    TC_API_BEGIN(ctx)
    shortest_unique_entry(ctx, text, n, sus_start, sus_len, false);
    TC_API_END(ctx)
}

int tc_shortest_unique_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t *d_sus_start, uint32_t *d_sus_len) {
    TC_API_BEGIN(ctx)
    shortest_unique_entry(ctx, d_text, n, d_sus_start, d_sus_len, true);
    TC_API_END(ctx)
}

// the repeat cover of a text: the bytes that lie in repeated content as spans, as a mask, and the text without them; the same over
// a caller's array of lengths (no counterpart in the reference): tc_cov_host.hpp
static CovCall cov_spans_call(uint32_t *span_start, uint32_t *span_len, uint64_t *nspans, uint64_t *covered) {
    CovCall c;
    c.what = COV_SPANS; c.span_start = span_start; c.span_len = span_len; c.count = nspans; c.covered = covered;
    return c;
}
static CovCall cov_mask_call(const uint8_t *map, uint8_t *out, uint64_t *covered) {
    CovCall c;
    c.what = COV_MASK; c.map = map; c.out = out; c.covered = covered;
    return c;
}
static CovCall cov_dedup_call(uint8_t *out, uint64_t *nout, uint64_t *covered) {
    CovCall c;
    c.what = COV_DEDUP; c.out = out; c.count = nout; c.covered = covered;
    return c;
}

int tc_repeat_spans(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind, uint32_t *span_start,
                    uint32_t *span_len, uint64_t *nspans, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    repeat_cover_entry(ctx, text, n, min_len, min_occ, kind, cov_spans_call(span_start, span_len, nspans, covered), false);
    TC_API_END(ctx)
}

int tc_repeat_spans_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind,
                        uint32_t *d_span_start, uint32_t *d_span_len, uint64_t *nspans, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    repeat_cover_entry(ctx, d_text, n, min_len, min_occ, kind, cov_spans_call(d_span_start, d_span_len, nspans, covered), true);
    TC_API_END(ctx)
}

int tc_repeat_mask(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind, const uint8_t *map,
                   uint8_t *out, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    repeat_cover_entry(ctx, text, n, min_len, min_occ, kind, cov_mask_call(map, out, covered), false);
    TC_API_END(ctx)
}

int tc_repeat_mask_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind, const uint8_t *map,
                       uint8_t *d_out, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    repeat_cover_entry(ctx, d_text, n, min_len, min_occ, kind, cov_mask_call(map, d_out, covered), true);
    TC_API_END(ctx)
}

int tc_repeat_dedup(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind, uint8_t *out,
                    uint64_t *nout, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    repeat_cover_entry(ctx, text, n, min_len, min_occ, kind, cov_dedup_call(out, nout, covered), false);
    TC_API_END(ctx)
}

int tc_repeat_dedup_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint32_t min_occ, uint32_t kind, uint8_t *d_out,
                        uint64_t *nout, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    repeat_cover_entry(ctx, d_text, n, min_len, min_occ, kind, cov_dedup_call(d_out, nout, covered), true);
    TC_API_END(ctx)
}

int tc_cover_spans_dev(tc_ctx *ctx, const uint32_t *d_len, uint64_t n, uint32_t min_len, uint32_t *d_span_start, uint32_t *d_span_len,
                       uint64_t *nspans, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    cover_entry(ctx, d_len, nullptr, n, min_len, cov_spans_call(d_span_start, d_span_len, nspans, covered));
    TC_API_END(ctx)
}

int tc_cover_mask_dev(tc_ctx *ctx, const uint32_t *d_len, const uint8_t *d_text, uint64_t n, uint32_t min_len, const uint8_t *map,
                      uint8_t *d_out, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    cover_entry(ctx, d_len, d_text, n, min_len, cov_mask_call(map, d_out, covered));
    TC_API_END(ctx)
}

int tc_cover_dedup_dev(tc_ctx *ctx, const uint32_t *d_len, const uint8_t *d_text, uint64_t n, uint32_t min_len, uint8_t *d_out,
                       uint64_t *nout, uint64_t *covered) {
    TC_API_BEGIN(ctx)
    cover_entry(ctx, d_len, d_text, n, min_len, cov_dedup_call(d_out, nout, covered));
    TC_API_END(ctx)
}

// the kept enhanced suffix array and its batched substring queries (no counterpart in the reference): tc_esa_host.hpp
int tc_esa_build(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_esa **out) {
    if (out) *out = nullptr;
    TC_API_BEGIN(ctx)
    esa_build_entry(ctx, text, n, out, false);
    TC_API_END(ctx)
}

int tc_esa_build_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_esa **out) {
    if (out) *out = nullptr;
    TC_API_BEGIN(ctx)
    esa_build_entry(ctx, d_text, n, out, true);
    TC_API_END(ctx)
}

void tc_esa_free(tc_esa *esa) { esa_release(esa); }
uint64_t tc_esa_n(const tc_esa *esa) { return esa ? esa->n : 0; }
uint64_t tc_esa_device_bytes(const tc_esa *esa, int part) { return esa_device_bytes(esa, part); }

int tc_esa_arrays(const tc_esa *esa, const uint8_t **d_text, const uint32_t **d_sa, const uint32_t **d_lcp, const uint32_t **d_isa) {
    if (!esa) return TC_ERR_ARG;
    if (d_text) *d_text = esa->d_text;
    if (d_sa) *d_sa = esa->d_sa;
    if (d_lcp) *d_lcp = esa->d_lcp;
    if (d_isa) *d_isa = esa->d_isa;
    return TC_OK;
}

int tc_esa_read(tc_ctx *ctx, const tc_esa *esa, int what, uint64_t first, uint64_t count, void *dst, int dst_on_device) {
    TC_API_BEGIN(ctx)
    esa_read_entry(ctx, esa, what, first, count, dst, dst_on_device != 0);
    TC_API_END(ctx)
}

int tc_esa_lce(tc_ctx *ctx, const tc_esa *esa, const uint32_t *a, const uint32_t *b, uint64_t nq, uint32_t max_mismatch, uint32_t *len,
               uint32_t *mm) {
    TC_API_BEGIN(ctx)
    esa_lce_entry(ctx, esa, a, b, nq, max_mismatch, len, mm, false);
    TC_API_END(ctx)
}

int tc_esa_lce_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_a, const uint32_t *d_b, uint64_t nq, uint32_t max_mismatch,
                   uint32_t *d_len, uint32_t *d_mm) {
    TC_API_BEGIN(ctx)
    esa_lce_entry(ctx, esa, d_a, d_b, nq, max_mismatch, d_len, d_mm, true);
    TC_API_END(ctx)
}

int tc_esa_find(tc_ctx *ctx, const tc_esa *esa, const uint32_t *start, const uint32_t *len, uint64_t nq, uint32_t *first_row, uint32_t *occ,
                uint32_t *first_pos) {
    TC_API_BEGIN(ctx)
    esa_find_entry(ctx, esa, start, len, nq, first_row, occ, first_pos, false);
    TC_API_END(ctx)
}

int tc_esa_find_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_start, const uint32_t *d_len, uint64_t nq, uint32_t *d_first_row,
                    uint32_t *d_occ, uint32_t *d_first_pos) {
    TC_API_BEGIN(ctx)
    esa_find_entry(ctx, esa, d_start, d_len, nq, d_first_row, d_occ, d_first_pos, true);
    TC_API_END(ctx)
}

int tc_esa_compare(tc_ctx *ctx, const tc_esa *esa, const uint32_t *a_start, const uint32_t *a_len, const uint32_t *b_start,
                   const uint32_t *b_len, uint64_t nq, int8_t *order, uint32_t *common) {
    TC_API_BEGIN(ctx)
    esa_compare_entry(ctx, esa, a_start, a_len, b_start, b_len, nq, reinterpret_cast<signed char *>(order), common, false);
    TC_API_END(ctx)
}

int tc_esa_compare_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_a_start, const uint32_t *d_a_len, const uint32_t *d_b_start,
                       const uint32_t *d_b_len, uint64_t nq, int8_t *d_order, uint32_t *d_common) {
    TC_API_BEGIN(ctx)
    esa_compare_entry(ctx, esa, d_a_start, d_a_len, d_b_start, d_b_len, nq, reinterpret_cast<signed char *>(d_order), d_common, true);
    TC_API_END(ctx)
}

// document collections on the kept enhanced suffix array (no counterpart in the reference): tc_esa_docs_host.hpp
int tc_esa_build_docs(tc_ctx *ctx, const uint8_t *text, uint64_t n, const uint32_t *doc_start, uint32_t ndocs, tc_esa **out) {
    if (out) *out = nullptr;
    TC_API_BEGIN(ctx)
    esa_build_docs_entry(ctx, text, n, doc_start, ndocs, out, false);
    TC_API_END(ctx)
}

int tc_esa_build_docs_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint32_t *doc_start, uint32_t ndocs, tc_esa **out) {
    if (out) *out = nullptr;
    TC_API_BEGIN(ctx)
    esa_build_docs_entry(ctx, d_text, n, doc_start, ndocs, out, true);
    TC_API_END(ctx)
}

uint32_t tc_esa_ndocs(const tc_esa *esa) { return esa ? esa->ndocs : 0; }

int tc_esa_doc_arrays(const tc_esa *esa, const uint32_t **d_doc_start, const uint32_t **d_da, const uint32_t **d_pv) {
    if (!esa || !esa->ndocs) return TC_ERR_ARG;
    if (d_doc_start) *d_doc_start = esa->d_doc_start;
    if (d_da) *d_da = esa->d_da;
    if (d_pv) *d_pv = esa->d_pv;
    return TC_OK;
}

int tc_esa_doc_count(tc_ctx *ctx, const tc_esa *esa, const uint32_t *start, const uint32_t *len, uint64_t nq, uint32_t limit, uint32_t *df,
                     uint32_t *occ) {
    TC_API_BEGIN(ctx)
    esa_doc_count_entry(ctx, esa, start, len, nq, limit, df, occ, false);
    TC_API_END(ctx)
}

int tc_esa_doc_count_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_start, const uint32_t *d_len, uint64_t nq, uint32_t limit,
                         uint32_t *d_df, uint32_t *d_occ) {
    TC_API_BEGIN(ctx)
    esa_doc_count_entry(ctx, esa, d_start, d_len, nq, limit, d_df, d_occ, true);
    TC_API_END(ctx)
}

int tc_esa_doc_list(tc_ctx *ctx, const tc_esa *esa, const uint32_t *start, const uint32_t *len, uint64_t nq, uint32_t limit,
                    uint64_t *list_offs, uint32_t *docs, uint32_t *hit_pos, uint64_t *ntotal) {
    TC_API_BEGIN(ctx)
    esa_doc_list_entry(ctx, esa, start, len, nq, limit, list_offs, docs, hit_pos, ntotal, false);
    TC_API_END(ctx)
}

int tc_esa_doc_list_dev(tc_ctx *ctx, const tc_esa *esa, const uint32_t *d_start, const uint32_t *d_len, uint64_t nq, uint32_t limit,
                        uint64_t *d_list_offs, uint32_t *d_docs, uint32_t *d_hit_pos, uint64_t *ntotal) {
    TC_API_BEGIN(ctx)
    esa_doc_list_entry(ctx, esa, d_start, d_len, nq, limit, d_list_offs, d_docs, d_hit_pos, ntotal, true);
    TC_API_END(ctx)
}

int tc_esa_kmer_docs(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint32_t min_df, uint32_t max_df, uint32_t *kmer_pos, uint32_t *kmer_occ,
                     uint32_t *kmer_df, uint32_t *kmer_row, uint64_t *nk) {
    TC_API_BEGIN(ctx)
    esa_kmer_docs_entry(ctx, esa, k, min_df, max_df, kmer_pos, kmer_occ, kmer_df, kmer_row, nk, false);
    TC_API_END(ctx)
}

int tc_esa_kmer_docs_dev(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint32_t min_df, uint32_t max_df, uint32_t *d_kmer_pos,
                         uint32_t *d_kmer_occ, uint32_t *d_kmer_df, uint32_t *d_kmer_row, uint64_t *nk) {
    TC_API_BEGIN(ctx)
    esa_kmer_docs_entry(ctx, esa, k, min_df, max_df, d_kmer_pos, d_kmer_occ, d_kmer_df, d_kmer_row, nk, true);
    TC_API_END(ctx)
}

int tc_esa_kmer_doc_spectrum(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint64_t *hist, uint64_t *distinct) {
    TC_API_BEGIN(ctx)
    esa_kmer_doc_spectrum_entry(ctx, esa, k, hist, distinct, false);
    TC_API_END(ctx)
}

int tc_esa_kmer_doc_spectrum_dev(tc_ctx *ctx, const tc_esa *esa, uint32_t k, uint64_t *d_hist, uint64_t *distinct) {
    TC_API_BEGIN(ctx)
    esa_kmer_doc_spectrum_entry(ctx, esa, k, d_hist, distinct, true);
    TC_API_END(ctx)
}

// cross-document matches on the kept enhanced suffix array (no counterpart in the reference): tc_esa_xdoc_host.hpp
int tc_esa_doc_match(tc_ctx *ctx, const tc_esa *esa, int kind, int clamp, uint32_t *xl, uint32_t *src, uint32_t *xdoc) {
    TC_API_BEGIN(ctx)
    esa_doc_match_entry(ctx, esa, kind, clamp, xl, src, xdoc, false);
    TC_API_END(ctx)
}

int tc_esa_doc_match_dev(tc_ctx *ctx, const tc_esa *esa, int kind, int clamp, uint32_t *d_xl, uint32_t *d_src, uint32_t *d_xdoc) {
    TC_API_BEGIN(ctx)
    esa_doc_match_entry(ctx, esa, kind, clamp, d_xl, d_src, d_xdoc, true);
    TC_API_END(ctx)
}

int tc_esa_doc_shared(tc_ctx *ctx, const tc_esa *esa, int kind, uint32_t min_len, uint64_t *shared, uint32_t *longest) {
    TC_API_BEGIN(ctx)
    esa_doc_shared_entry(ctx, esa, kind, min_len, shared, longest, false);
    TC_API_END(ctx)
}

int tc_esa_doc_shared_dev(tc_ctx *ctx, const tc_esa *esa, int kind, uint32_t min_len, uint64_t *d_shared, uint32_t *d_longest) {
    TC_API_BEGIN(ctx)
    esa_doc_shared_entry(ctx, esa, kind, min_len, d_shared, d_longest, true);
    TC_API_END(ctx)
}

int tc_longest_palindrome(tc_ctx *ctx, const uint8_t *text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch, uint32_t *start,
                          uint32_t *len, uint32_t *mm) {
    TC_API_BEGIN(ctx)
    longest_palindrome_entry(ctx, text, n, comp, max_mismatch, start, len, mm, false);
    TC_API_END(ctx)
}

int tc_longest_palindrome_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, const uint8_t *comp, uint32_t max_mismatch,
                              uint32_t *start, uint32_t *len, uint32_t *mm) {
    TC_API_BEGIN(ctx)
    longest_palindrome_entry(ctx, d_text, n, comp, max_mismatch, start, len, mm, true);
    TC_API_END(ctx)
}

// the k-mers of a text, their abundance spectrum and the all-k profile (no counterpart in the reference): tc_kmer_host.hpp
int tc_kmers(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ, uint32_t *sa,
             uint32_t *kmer_pos, uint32_t *kmer_occ, uint32_t *kmer_row, uint64_t *nk) {
    TC_API_BEGIN(ctx)
    kmers_entry(ctx, text, n, k, min_occ, max_occ, sa, kmer_pos, kmer_occ, kmer_row, nk, false);
    TC_API_END(ctx)
}

int tc_kmers_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t k, uint32_t min_occ, uint32_t max_occ, uint32_t *d_sa,
                 uint32_t *d_kmer_pos, uint32_t *d_kmer_occ, uint32_t *d_kmer_row, uint64_t *nk) {
    TC_API_BEGIN(ctx)
    kmers_entry(ctx, d_text, n, k, min_occ, max_occ, d_sa, d_kmer_pos, d_kmer_occ, d_kmer_row, nk, true);
    TC_API_END(ctx)
}

int tc_kmers_esa_dev(tc_ctx *ctx, const uint32_t *d_sa, const uint32_t *d_lcp, uint64_t N, uint32_t k, uint32_t min_occ,
                     uint32_t max_occ, uint32_t *d_kmer_pos, uint32_t *d_kmer_occ, uint32_t *d_kmer_row, uint64_t *nk) {
    TC_API_BEGIN(ctx)
    kmers_esa_entry(ctx, d_sa, d_lcp, N, k, min_occ, max_occ, d_kmer_pos, d_kmer_occ, d_kmer_row, nk);
    TC_API_END(ctx)
}

int tc_kmer_spectrum(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t k, uint32_t bins, uint64_t *hist, uint64_t *distinct,
                     uint64_t *total) {
    TC_API_BEGIN(ctx)
    kmer_spectrum_entry(ctx, text, n, k, bins, hist, distinct, total);
    TC_API_END(ctx)
}

int tc_kmer_spectrum_esa_dev(tc_ctx *ctx, const uint32_t *d_sa, const uint32_t *d_lcp, uint64_t N, uint32_t k, uint32_t bins,
                             uint64_t *d_hist, uint64_t *distinct, uint64_t *total) {
    TC_API_BEGIN(ctx)
    kmer_spectrum_esa_entry(ctx, d_sa, d_lcp, N, k, bins, d_hist, distinct, total);
    TC_API_END(ctx)
}

int tc_kmer_profile(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t kmax, uint64_t *distinct, uint64_t *unique) {
    TC_API_BEGIN(ctx)
    kmer_profile_entry(ctx, text, n, kmax, distinct, unique);
    TC_API_END(ctx)
}

int tc_kmer_profile_esa_dev(tc_ctx *ctx, const uint32_t *d_lcp, uint64_t N, uint32_t kmax, uint64_t *distinct, uint64_t *unique) {
    TC_API_BEGIN(ctx)
    kmer_profile_esa_entry(ctx, d_lcp, N, kmax, distinct, unique);
    TC_API_END(ctx)
}

// one text against another: matching statistics, maximal exact matches, longest common substring (no counterpart in the
// reference): tc_tm_host.hpp
int tc_text_match_stats(tc_ctx *ctx, const uint8_t *query, uint64_t a, const uint8_t *target, uint64_t b, uint32_t *ms_len,
                        uint32_t *ms_pos, uint32_t *ms_occ) {
    TC_API_BEGIN(ctx)
    text_match_stats_entry(ctx, query, a, target, b, ms_len, ms_pos, ms_occ, false);
    TC_API_END(ctx)
}

int tc_text_match_stats_dev(tc_ctx *ctx, const uint8_t *d_query, uint64_t a, const uint8_t *d_target, uint64_t b, uint32_t *d_ms_len,
                            uint32_t *d_ms_pos, uint32_t *d_ms_occ) {
    TC_API_BEGIN(ctx)
    text_match_stats_entry(ctx, d_query, a, d_target, b, d_ms_len, d_ms_pos, d_ms_occ, true);
    TC_API_END(ctx)
}

int tc_text_mems(tc_ctx *ctx, const uint8_t *query, uint64_t a, const uint8_t *target, uint64_t b, uint32_t min_len,
                 uint32_t *mem_start, uint32_t *mem_pos, uint32_t *mem_len, uint64_t *nmem) {
    TC_API_BEGIN(ctx)
    text_mems_entry(ctx, query, a, target, b, min_len, mem_start, mem_pos, mem_len, nmem, false);
    TC_API_END(ctx)
}

int tc_text_mems_dev(tc_ctx *ctx, const uint8_t *d_query, uint64_t a, const uint8_t *d_target, uint64_t b, uint32_t min_len,
                     uint32_t *d_mem_start, uint32_t *d_mem_pos, uint32_t *d_mem_len, uint64_t *nmem) {
    TC_API_BEGIN(ctx)
    text_mems_entry(ctx, d_query, a, d_target, b, min_len, d_mem_start, d_mem_pos, d_mem_len, nmem, true);
    TC_API_END(ctx)
}

int tc_text_lcs(tc_ctx *ctx, const uint8_t *query, uint64_t a, const uint8_t *target, uint64_t b, uint32_t *len, uint64_t *qpos,
                uint64_t *tpos, uint64_t *sum) {
    TC_API_BEGIN(ctx)
    text_lcs_entry(ctx, query, a, target, b, len, qpos, tpos, sum, false);
    TC_API_END(ctx)
}

int tc_text_lcs_dev(tc_ctx *ctx, const uint8_t *d_query, uint64_t a, const uint8_t *d_target, uint64_t b, uint32_t *len,
                    uint64_t *qpos, uint64_t *tpos, uint64_t *sum) {
    TC_API_BEGIN(ctx)
    text_lcs_entry(ctx, d_query, a, d_target, b, len, qpos, tpos, sum, true);
    TC_API_END(ctx)
}

int tc_mems_from_stats_dev(tc_ctx *ctx, const uint32_t *d_ms_len, const uint32_t *d_ms_pos, uint64_t a, uint32_t min_len,
                           uint32_t *d_mem_start, uint32_t *d_mem_pos, uint32_t *d_mem_len, uint64_t *nmem) {
    TC_API_BEGIN(ctx)
    mems_from_stats_entry(ctx, d_ms_len, d_ms_pos, a, min_len, d_mem_start, d_mem_pos, d_mem_len, nmem);
    TC_API_END(ctx)
}

// ================================================================= Data.MTF
int tc_mtf_encode(tc_ctx *ctx, const uint8_t *L, uint64_t N, int64_t primary, uint16_t *idx,
                  int16_t *final_list, uint32_t *sigma) {
    TC_API_BEGIN(ctx)
    mtf_encode_entry(ctx, L, N, primary, idx, final_list, sigma);
    TC_API_END(ctx)
}

int tc_mtf_encode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint16_t *idx,
                      int16_t *final_list, uint32_t *sigma) {
    TC_API_BEGIN(ctx)
    mtf_encode_sym_entry(ctx, sym, N, idx, final_list, sigma);
    TC_API_END(ctx)
}

// ================================================================= Data.RLE
int tc_rle_encode(tc_ctx *ctx, const uint8_t *L, uint64_t N, int64_t primary, uint32_t *counts,
                  int16_t *syms, uint64_t *nruns) {
    TC_API_BEGIN(ctx)
    rle_encode_entry(ctx, L, N, primary, counts, syms, nruns);
    TC_API_END(ctx)
}

int tc_rle_encode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint32_t *counts,
                      int16_t *syms, uint64_t *nruns) {
    TC_API_BEGIN(ctx)
    rle_encode_vals_entry<SymAcc, i16>(ctx, sym, N, counts, syms, nruns);
    TC_API_END(ctx)
}

int tc_rle_encode_u16(tc_ctx *ctx, const uint16_t *vals, uint64_t N, uint32_t *counts,
                      uint16_t *run_vals, uint64_t *nruns) {
    TC_API_BEGIN(ctx)
    rle_encode_vals_entry<U16Acc, u16>(ctx, vals, N, counts, run_vals, nruns);
    TC_API_END(ctx)
}

// ============================================================ fused pipeline (the bodies: tc_hostio_host.hpp)
int tc_encode_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_block *out) {
    TC_API_BEGIN(ctx)
    encode_entry(ctx, d_text, n, out, true);
    TC_API_END(ctx)
}

int tc_encode(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_block *out) {
    TC_API_BEGIN(ctx)
    encode_entry(ctx, text, n, out, false);
    TC_API_END(ctx)
}

// ============================================================ synthetic input (tc_generate.hpp)
int tc_generate_dev(tc_ctx *ctx, int kind, uint64_t seed, uint64_t n, uint8_t *d_out) {
    TC_API_BEGIN(ctx)
    generate_entry(ctx, kind, seed, n, d_out);
    TC_API_END(ctx)
}

// ===================================================================== decode
int tc_bwt_decode(tc_ctx *ctx, const uint8_t *L, uint64_t N, uint64_t primary, uint8_t *text) {
    TC_API_BEGIN(ctx)
    bwt_decode_entry(ctx, L, N, primary, text);
    TC_API_END(ctx)
}

int tc_bwt_decode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint8_t *text, uint64_t *n_out) {
    TC_API_BEGIN(ctx)
    bwt_decode_sym_entry(ctx, sym, N, text, n_out);
    TC_API_END(ctx)
}

int tc_mtf_decode(tc_ctx *ctx, const uint16_t *idx, uint64_t N, const int16_t *list,
                  uint32_t nlist, int16_t *sym) {
    TC_API_BEGIN(ctx)
    mtf_decode_entry(ctx, idx, N, list, nlist, sym);
    TC_API_END(ctx)
}

int tc_rle_decode(tc_ctx *ctx, const uint32_t *counts, const int16_t *syms, uint64_t nruns,
                  int16_t *sym_out, uint64_t *N) {
    TC_API_BEGIN(ctx)
    rle_decode_entry<i16>(ctx, counts, syms, nruns, sym_out, N);
    TC_API_END(ctx)
}

int tc_rle_decode_u16(tc_ctx *ctx, const uint32_t *counts, const uint16_t *run_vals,
                      uint64_t nruns, uint16_t *vals_out, uint64_t *N) {
    TC_API_BEGIN(ctx)
    rle_decode_entry<u16>(ctx, counts, run_vals, nruns, vals_out, N);
    TC_API_END(ctx)
}

int tc_decode_dev(tc_ctx *ctx, const tc_block *blk, uint8_t *d_text) {
    TC_API_BEGIN(ctx)
    decode_entry(ctx, blk, d_text, true);
    TC_API_END(ctx)
}

int tc_decode(tc_ctx *ctx, const tc_block *blk, uint8_t *text) {
    TC_API_BEGIN(ctx)
    decode_entry(ctx, blk, text, false);
    TC_API_END(ctx)
}

// =============================== encoded-block wire format and container (host side: tc_container_host.hpp)
uint64_t tc_block_packed_bound(uint64_t nruns, uint32_t sigma) {
    const int fmt = pack_format(sigma);
    // nibble stream: <= 1 byte per run + 16 bytes of padding per packer tile + 4-byte escapes
    if (fmt == 0) return nruns + 16 * ((nruns + PK_TILE - 1) / PK_TILE + 1) + 4 * nruns;
    // bytes + 8-byte alignment + worst-case escape list (every run escaping)
    return (((u64)fmt * nruns + 7) & ~7ull) + 8 * nruns + 8;
}

int tc_block_pack_dev(tc_ctx *ctx, const tc_block *blk, uint8_t *d_packed, uint64_t *packed_bytes,
                      uint64_t *nesc) {
    TC_API_BEGIN(ctx)
    block_pack_device(ctx, blk, d_packed, packed_bytes, nesc);
    TC_API_END(ctx)
}

int tc_block_unpack_dev(tc_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, uint64_t nruns,
                        uint32_t sigma, uint64_t nesc, tc_block *blk) {
    TC_API_BEGIN(ctx)
    block_unpack_device(ctx, d_packed, packed_bytes, nruns, sigma, nesc, blk);
    TC_API_END(ctx)
}

uint64_t tc_container_bound(uint64_t nruns, uint32_t sigma) {
    return TC_CONTAINER_HEADER + tc_block_packed_bound(nruns, sigma);
}

int tc_encode_container_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint8_t *d_out, uint64_t *bytes) {
    TC_API_BEGIN(ctx)
    encode_container_dev_entry(ctx, d_text, n, d_out, bytes);
    TC_API_END(ctx)
}

int tc_block_to_container_dev(tc_ctx *ctx, const tc_block *blk, uint8_t *d_out, uint64_t *bytes) {
    TC_API_BEGIN(ctx)
    container_write_device(ctx, blk, d_out, bytes);
    TC_API_END(ctx)
}

int tc_container_to_block_dev(tc_ctx *ctx, const uint8_t *d_in, uint64_t bytes, tc_block *blk) {
    TC_API_BEGIN(ctx)
    container_read_device(ctx, d_in, bytes, blk);
    TC_API_END(ctx)
}

int tc_container_info(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, uint64_t *n, uint64_t *nruns) {
    if (!ctx) return TC_ERR_ARG;
    try {
        if (!container || bytes < TC_CONTAINER_HEADER) TC_FAIL(ctx, TC_ERR_MALFORMED, "container shorter than its header");
        const ContainerHeader h = container_header_parse(ctx, container, bytes, HDR_MAGIC);
        if (n) *n = h.n;
        if (nruns) *nruns = h.nruns;
        return TC_OK;
    } catch (const TcFail &f) {
        return f.code;
    }
}

int tc_container_coding(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, int *coding) {
    if (!ctx) return TC_ERR_ARG;
    try {
        if (!coding) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
        if (!container || bytes < TC_CONTAINER_HEADER) TC_FAIL(ctx, TC_ERR_MALFORMED, "container shorter than its header");
        const ContainerHeader h = container_header_parse(ctx, container, bytes, HDR_MAGIC);
        if (h.format == HF_FORMAT) *coding = TC_CODING_HUFFMAN;
        else if (h.sigma <= TC_MAX_SIGMA && h.format == (u32)pack_format(h.sigma)) *coding = TC_CODING_PACKED;
        else TC_FAIL(ctx, TC_ERR_MALFORMED, "container header names no known body format");
        return TC_OK;
    } catch (const TcFail &f) {
        return f.code;
    }
}

int tc_encode_container(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t *bytes) {
    TC_API_BEGIN(ctx)
    encode_container_entry(ctx, text, n, out, bytes);
    TC_API_END(ctx)
}

int tc_decode_container(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, uint8_t *text, uint64_t *n_out) {
    TC_API_BEGIN(ctx)
    decode_container_entry(ctx, container, bytes, text, n_out);
    TC_API_END(ctx)
}

// ================================================== chunked stream of containers (tc_hostio_host.hpp)
uint64_t tc_stream_bound(uint64_t n, uint64_t block_bytes) {
    if (block_bytes == 0) block_bytes = TC_STREAM_BLOCK_DEFAULT;
    if (block_bytes > TC_MAX_N) block_bytes = TC_MAX_N;
    const u64 nb = stream_blocks(n, block_bytes);
    const u64 last = n - (nb - 1) * block_bytes;
    return (nb - 1) * container_bound_any(block_bytes) + container_bound_any(last);
}

int tc_encode_stream(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t block_bytes, uint8_t *out,
                     uint64_t *bytes) {
    TC_API_BEGIN(ctx)
    encode_stream_entry(ctx, text, n, block_bytes, out, bytes);
    TC_API_END(ctx)
}

int tc_stream_info(tc_ctx *ctx, const uint8_t *stream, uint64_t bytes, uint64_t *n_total, uint64_t *nblocks) {
    if (!ctx) return TC_ERR_ARG;
    try {
        const StreamIndex ix = stream_index(ctx, stream, bytes);
        if (n_total) *n_total = ix.n_total;
        if (nblocks) *nblocks = ix.off.size();
        return TC_OK;
    } catch (const TcFail &f) {
        return f.code;
    }
}

int tc_decode_stream(tc_ctx *ctx, const uint8_t *stream, uint64_t bytes, uint8_t *text, uint64_t *n_out) {
    TC_API_BEGIN(ctx)
    decode_stream_entry(ctx, stream, bytes, text, n_out);
    TC_API_END(ctx)
}

// =============================================================== Data.FMIndex (the bodies: tc_fm_host.hpp)
int tc_fm_build(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, text, nullptr, n, 1, 0, 0, out);
    TC_API_END(ctx)
}

int tc_fm_build_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, nullptr, d_text, n, 1, 0, 0, out);
    TC_API_END(ctx)
}

int tc_fm_build_sampled(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sa_rate, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, text, nullptr, n, sa_rate, 0, 1, out);
    TC_API_END(ctx)
}

int tc_fm_build_sampled_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t sa_rate, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, nullptr, d_text, n, sa_rate, 0, 1, out);
    TC_API_END(ctx)
}

int tc_fm_build_self(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, text, nullptr, n, sa_rate, text_rate, 2, out);
    TC_API_END(ctx)
}

int tc_fm_build_self_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, nullptr, d_text, n, sa_rate, text_rate, 2, out);
    TC_API_END(ctx)
}

int tc_fm_build_lcp(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, text, nullptr, n, sa_rate, text_rate, 2, out, true);
    TC_API_END(ctx)
}

int tc_fm_build_lcp_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, uint32_t sa_rate, uint32_t text_rate, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_build_entry(ctx, nullptr, d_text, n, sa_rate, text_rate, 2, out, true);
    TC_API_END(ctx)
}

int tc_fm_has_lcp(const tc_fm *fm) { return fm && fm->d_lcp ? 1 : 0; }
uint32_t tc_fm_sa_rate(const tc_fm *fm) { return fm ? fm->sa_rate : 0; }
uint32_t tc_fm_text_rate(const tc_fm *fm) { return fm ? fm->text_rate : 0; }
uint64_t tc_fm_device_bytes(const tc_fm *fm, int part) { return fm_device_bytes(fm, part); }
void tc_fm_free(tc_fm *fm) { fm_release(fm); }

uint64_t tc_fm_export_bound(const tc_fm *fm, int with_locate) { return fm_export_bound(fm, with_locate); }

int tc_fm_export_dev(tc_ctx *ctx, const tc_fm *fm, int with_locate, uint8_t *d_out, uint64_t *bytes) {
    TC_API_BEGIN(ctx)
    fm_export_device(ctx, fm, with_locate, d_out, bytes);
    TC_API_END(ctx)
}

int tc_fm_import_dev(tc_ctx *ctx, const uint8_t *d_in, uint64_t bytes, tc_fm **out) {
    TC_API_BEGIN(ctx)
    fm_import_device(ctx, d_in, bytes, out);
    TC_API_END(ctx)
}

int tc_fm_count_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs,
                    uint64_t npat, int64_t *d_out) {
    TC_API_BEGIN(ctx)
    fm_count_entry(ctx, fm, d_pats, d_offs, npat, true, 0, d_out, true);
    TC_API_END(ctx)
}

int tc_fm_count(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs,
                uint64_t npat, int64_t *out) {
    TC_API_BEGIN(ctx)
    fm_count_entry(ctx, fm, pats, offs, npat, true, 0, out, false);
    TC_API_END(ctx)
}

int tc_fm_locate(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs,
                 uint64_t npat, uint64_t *hit_offs, uint64_t *hits, uint64_t *nhits) {
    TC_API_BEGIN(ctx)
    fm_locate_entry(ctx, fm, pats, offs, npat, true, 0, hit_offs, hits, nullptr, nhits, false);
    TC_API_END(ctx)
}

int tc_fm_locate_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs,
                     uint64_t npat, uint64_t *d_hit_offs, uint64_t *d_hits, uint64_t *nhits) {
    TC_API_BEGIN(ctx)
    fm_locate_entry(ctx, fm, d_pats, d_offs, npat, true, 0, d_hit_offs, d_hits, nullptr, nhits, true);
    TC_API_END(ctx)
}

// ---- search with mismatches (the kernel: tc_fm_mm.hpp) ---------------------------------
int tc_fm_count_mm_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t k,
                       int64_t *d_out) {
    TC_API_BEGIN(ctx)
    fm_count_entry(ctx, fm, d_pats, d_offs, npat, false, k, d_out, true);
    TC_API_END(ctx)
}

int tc_fm_count_mm(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t k,
                   int64_t *out) {
    TC_API_BEGIN(ctx)
    fm_count_entry(ctx, fm, pats, offs, npat, false, k, out, false);
    TC_API_END(ctx)
}

int tc_fm_locate_mm(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t k,
                    uint64_t *hit_offs, uint64_t *hits, uint8_t *hit_mm, uint64_t *nhits) {
    TC_API_BEGIN(ctx)
    fm_locate_entry(ctx, fm, pats, offs, npat, false, k, hit_offs, hits, hit_mm, nhits, false);
    TC_API_END(ctx)
}

int tc_fm_locate_mm_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t k,
                        uint64_t *d_hit_offs, uint64_t *d_hits, uint8_t *d_hit_mm, uint64_t *nhits) {
    TC_API_BEGIN(ctx)
    fm_locate_entry(ctx, fm, d_pats, d_offs, npat, false, k, d_hit_offs, d_hits, d_hit_mm, nhits, true);
    TC_API_END(ctx)
}

int tc_fm_extract_dev(tc_ctx *ctx, const tc_fm *fm, const uint64_t *d_starts, const uint64_t *d_lens, uint64_t nq,
                      uint64_t *d_out_offs, uint8_t *d_out, uint64_t *nbytes) {
    TC_API_BEGIN(ctx)
    fm_extract_entry(ctx, fm, d_starts, d_lens, nq, d_out_offs, d_out, nbytes, true);
    TC_API_END(ctx)
}

int tc_fm_extract(tc_ctx *ctx, const tc_fm *fm, const uint64_t *starts, const uint64_t *lens, uint64_t nq,
                  uint64_t *out_offs, uint8_t *out, uint64_t *nbytes) {
    TC_API_BEGIN(ctx)
    fm_extract_entry(ctx, fm, starts, lens, nq, out_offs, out, nbytes, false);
    TC_API_END(ctx)
}

// ---- factorize / unfactorize (the kernels: tc_fm_factor.hpp) ---------------------------
int tc_fm_factorize(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint64_t *fac_offs,
                    uint64_t *fac_pos, uint32_t *fac_len, uint64_t *nfac) {
    TC_API_BEGIN(ctx)
    fm_factor_entry(ctx, fm, pats, offs, npat, fac_offs, fac_pos, fac_len, nfac, false);
    TC_API_END(ctx)
}

int tc_fm_factorize_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat,
                        uint64_t *d_fac_offs, uint64_t *d_fac_pos, uint32_t *d_fac_len, uint64_t *nfac) {
    TC_API_BEGIN(ctx)
    fm_factor_entry(ctx, fm, d_pats, d_offs, npat, d_fac_offs, d_fac_pos, d_fac_len, nfac, true);
    TC_API_END(ctx)
}

int tc_fm_unfactorize(tc_ctx *ctx, const tc_fm *fm, const uint64_t *fac_offs, const uint64_t *fac_pos, const uint32_t *fac_len,
                      uint64_t npat, uint64_t *out_offs, uint8_t *out, uint64_t *nbytes) {
    TC_API_BEGIN(ctx)
    fm_unfactor_entry(ctx, fm, fac_offs, fac_pos, fac_len, npat, out_offs, out, nbytes, false);
    TC_API_END(ctx)
}

int tc_fm_unfactorize_dev(tc_ctx *ctx, const tc_fm *fm, const uint64_t *d_fac_offs, const uint64_t *d_fac_pos,
                          const uint32_t *d_fac_len, uint64_t npat, uint64_t *d_out_offs, uint8_t *d_out, uint64_t *nbytes) {
    TC_API_BEGIN(ctx)
    fm_unfactor_entry(ctx, fm, d_fac_offs, d_fac_pos, d_fac_len, npat, d_out_offs, d_out, nbytes, true);
    TC_API_END(ctx)
}

// ---- matching statistics / maximal exact matches (the kernels: tc_fm_ms.hpp) -------------
int tc_fm_match_stats(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t *ms_len,
                      uint64_t *ms_pos, uint32_t *ms_occ) {
    TC_API_BEGIN(ctx)
    fm_match_stats_entry(ctx, fm, pats, offs, npat, ms_len, ms_pos, ms_occ, false);
    TC_API_END(ctx)
}

int tc_fm_match_stats_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat,
                          uint32_t *d_ms_len, uint64_t *d_ms_pos, uint32_t *d_ms_occ) {
    TC_API_BEGIN(ctx)
    fm_match_stats_entry(ctx, fm, d_pats, d_offs, npat, d_ms_len, d_ms_pos, d_ms_occ, true);
    TC_API_END(ctx)
}

int tc_fm_mems(tc_ctx *ctx, const tc_fm *fm, const uint8_t *pats, const uint64_t *offs, uint64_t npat, uint32_t min_len,
               uint64_t *mem_offs, uint64_t *mem_start, uint64_t *mem_pos, uint32_t *mem_len, uint64_t *nmem) {
    TC_API_BEGIN(ctx)
    fm_mems_entry(ctx, fm, pats, offs, npat, min_len, mem_offs, mem_start, mem_pos, mem_len, nmem, false);
    TC_API_END(ctx)
}

int tc_fm_mems_dev(tc_ctx *ctx, const tc_fm *fm, const uint8_t *d_pats, const uint64_t *d_offs, uint64_t npat, uint32_t min_len,
                   uint64_t *d_mem_offs, uint64_t *d_mem_start, uint64_t *d_mem_pos, uint32_t *d_mem_len, uint64_t *nmem) {
    TC_API_BEGIN(ctx)
    fm_mems_entry(ctx, fm, d_pats, d_offs, npat, min_len, d_mem_offs, d_mem_start, d_mem_pos, d_mem_len, nmem, true);
    TC_API_END(ctx)
}

int tc_fm_info(const tc_fm *fm, uint64_t *N, uint32_t *sigma, int16_t *c_sym, uint64_t *c_val,
               uint64_t *primary) {
    return fm_info(fm, N, sigma, c_sym, c_val, primary);
}

// ======================================================== multi-GPU exchange (RCCL, bound at run time: tc_comm.hpp)
int tc_comm_unique_id(tc_ctx *ctx, uint8_t *id) {
    TC_API_BEGIN(ctx)
    comm_unique_id_entry(ctx, id);
    TC_API_END(ctx)
}

int tc_comm_create(tc_ctx *ctx, const uint8_t *id, int rank, int world, tc_comm **out) {
    TC_API_BEGIN(ctx)
    comm_create_entry(ctx, id, rank, world, out);
    TC_API_END(ctx)
}

void tc_comm_destroy(tc_comm *comm) { comm_destroy_entry(comm); }

int tc_comm_reserved_cus(const tc_comm *comm) { return comm ? comm->cus : 0; }

int tc_comm_wait(tc_comm *c) {
    if (!c) return TC_ERR_ARG;
    tc_ctx *ctx = c->ctx;
    TC_API_BEGIN(ctx)
    comm_wait_entry(ctx, c);
    TC_API_END(ctx)
}

int tc_comm_gather(tc_comm *c, int root, const uint8_t *d_container, uint64_t bytes, uint8_t *d_recv,
                   uint64_t slot_bytes, uint64_t *sizes) {
    if (!c) return TC_ERR_ARG;
    tc_ctx *ctx = c->ctx;
    TC_API_BEGIN(ctx)
    comm_gather_entry(ctx, c, root, d_container, bytes, d_recv, slot_bytes, sizes);
    TC_API_END(ctx)
}

int tc_comm_broadcast(tc_comm *c, int root, uint8_t *d_buf, uint64_t bytes) {
    if (!c) return TC_ERR_ARG;
    tc_ctx *ctx = c->ctx;
    TC_API_BEGIN(ctx)
    comm_broadcast_entry(ctx, c, root, d_buf, bytes);
    TC_API_END(ctx)
}

// ======================================================== calibration and debug (textcomp_debug.h; tc_dbg_host.hpp)
int tc_dbg_checksum64_dev(tc_ctx *ctx, const void *d_p, uint64_t bytes, uint64_t *out) {
    TC_API_BEGIN(ctx)
    dbg_checksum64_entry(ctx, d_p, bytes, out);
    TC_API_END(ctx)
}

int tc_dbg_stream_bench(tc_ctx *ctx, uint64_t bytes, int width, int mode, int iters, double *gbps) {
    TC_API_BEGIN(ctx)
    dbg_stream_bench_entry(ctx, bytes, width, mode, iters, gbps);
    TC_API_END(ctx)
}

int tc_dbg_scatter_bench(tc_ctx *ctx, uint64_t n, uint32_t bins, uint32_t xrun, int iters, double *ms_per_pass) {
    TC_API_BEGIN(ctx)
    dbg_scatter_bench_entry(ctx, n, bins, xrun, iters, ms_per_pass);
    TC_API_END(ctx)
}

int tc_dbg_lcp_set_short_cap(tc_ctx *ctx, uint32_t cap) {
    if (!ctx) return TC_ERR_ARG;
    if (cap != 0 && (cap < 16 || cap > 65536 || cap % 16 != 0)) {
        ctx->err = "the short cap is a multiple of 16 in 16 .. 65536, or 0";
        return TC_ERR_ARG;
    }
    ctx->lcp_cap = cap;
    return TC_OK;
}

int tc_dbg_fm_set_lcp_fanout(tc_ctx *ctx, uint32_t fanout) {
    if (!ctx) return TC_ERR_ARG;
    if (fanout != 4 && fanout != 8 && fanout != 16 && fanout != 64) {
        ctx->err = "the fan-out of the LCP min tree is 4, 8, 16 or 64";
        return TC_ERR_ARG;
    }
    ctx->fm_lcp_fanout = fanout;
    return TC_OK;
}

int tc_dbg_lz_set_tile(tc_ctx *ctx, uint32_t tile) {
    if (!ctx) return TC_ERR_ARG;
    if (tile != 0 && (tile < 64 || tile > LZ_TILE_MAX || (tile & (tile - 1)) != 0)) {
        ctx->err = "the tile of the LZ77 parse is a power of two in 64 .. 16384, or 0";
        return TC_ERR_ARG;
    }
    ctx->lz_tile = tile;
    return TC_OK;
}

int tc_dbg_msd_split_used(tc_ctx *ctx, uint32_t *used) {
    if (!ctx || !used) return TC_ERR_ARG;
    *used = ctx->msd_split_used ? 1u : 0u;
    return TC_OK;
}

int tc_dbg_msd_dir(tc_ctx *ctx, uint32_t out[2]) {
    TC_API_BEGIN(ctx)
    if (!out) TC_FAIL(ctx, TC_ERR_ARG, "out is null");
    sa_dbg_msd_dir(ctx, out);
    TC_API_END(ctx)
}

int tc_dbg_tied_probe(tc_ctx *ctx, uint32_t out[2]) {
    if (!ctx || !out) return TC_ERR_ARG;
    out[0] = (uint32_t)ctx->tied_probe_used;
    out[1] = ctx->tied_probe_found;
    return TC_OK;
}

int tc_dbg_ibwt_walk(tc_ctx *ctx, uint32_t out[3]) {
    if (!ctx || !out) return TC_ERR_ARG;
    out[0] = ctx->ibwt_attempts;
    out[1] = ctx->ibwt_overflowed;
    out[2] = ctx->ibwt_extra_taken;
    return TC_OK;
}

int tc_dbg_dispatch_probe(tc_ctx *ctx, uint32_t grid, uint32_t lds_bytes, uint32_t spin_cycles, uint32_t *out6) {
    TC_API_BEGIN(ctx)
    dbg_dispatch_probe_entry(ctx, grid, lds_bytes, spin_cycles, out6);
    TC_API_END(ctx)
}

int tc_dbg_sort_bench(tc_ctx *ctx, uint64_t n, int key_bits, int iters, int check, double *ms_per_pass) {
    TC_API_BEGIN(ctx)
    dbg_sort_bench_entry(ctx, n, key_bits, iters, check, ms_per_pass);
    TC_API_END(ctx)
}

int tc_dbg_seg_sort(tc_ctx *ctx, uint64_t *keys, uint32_t *vals, uint32_t m, int rbits, uint32_t levels[16]) {
    TC_API_BEGIN(ctx)
    dbg_seg_sort_entry(ctx, keys, vals, m, rbits, levels);
    TC_API_END(ctx)
}

int tc_dbg_tied_small(tc_ctx *ctx, int mode, uint32_t *slot, uint32_t *idx, uint32_t *grp, uint32_t m, uint32_t *t_idx,
                      uint32_t *t_rank, uint32_t *tpos) {
    TC_API_BEGIN(ctx)
    dbg_tied_small_entry(ctx, mode, slot, idx, grp, m, t_idx, t_rank, tpos);
    TC_API_END(ctx)
}

}  // extern "C"
