// tc_container_host.hpp -- host side of the wire format: the run packers, the container header, the Huffman
// body, text -> container on the device with its seal kernels, and the index of a chunked stream (kernels
// of the bodies: tc_pack.hpp, tc_huff.hpp).  Included by textcomp.hip only.
#pragma once
#include <vector>

#include "tc_encode_host.hpp"
#include "tc_pack.hpp"
#include "tc_huff.hpp"

// ====================================================== encoded-block wire format
// at most `nibbles` nibbles go into a nibble body of `cap` bytes: tiles meet inside 16-byte units and complete them
// by atomicOr, so that much of the body must start out zero
static void nib_body_zero(tc_ctx *ctx, u8 *body, u64 nibbles, u64 cap) {
    const u64 most = ((nibbles + 31) / 32 + 1) * 16;
    tc_memset_async(ctx, body, 0, most < (cap & ~15ull) ? most : (cap & ~15ull));
}

// ws_base: bytes at the start of the context's workspace that belong to the caller (the packer's scratch is
// carved behind them; the caller has reserved block_pack_scratch() bytes there, so the workspace never moves)
static size_t block_pack_scratch(u64 nruns) {
    return (((size_t)(nruns / PR_TILE + nruns / PK_TILE + 8) * sizeof(u64) + 255) & ~(size_t)255) +
           (((size_t)(nruns + 8) * sizeof(u32) + 255) & ~(size_t)255) + 512;
}
// the same for a context whose containers are Huffman-coded: the Huffman writer's scratch, or -- when the record falls
// back to the packing -- the packer's, one after the other in the same place
static size_t huff_scratch(u64 nruns) {
    const size_t nchunks = (size_t)(nruns / HF_K + 1);
    return (((size_t)HF_HIST_WORDS * sizeof(u32) + 255) & ~(size_t)255) + (((nchunks + 4) * sizeof(u32) + 255) & ~(size_t)255) +
           (((nchunks + 2) * sizeof(u64) + 255) & ~(size_t)255);
}
static size_t container_scratch(const tc_ctx *ctx, u64 nruns) {
    const size_t p = block_pack_scratch(nruns);
    if (ctx->coding != TC_CODING_HUFFMAN) return p;
    const size_t h = huff_scratch(nruns);
    return p > h ? p : h;
}
static void block_pack_device(tc_ctx *ctx, const tc_block *blk, uint8_t *d_packed, uint64_t *packed_bytes,
                              uint64_t *nesc, size_t ws_base = 0) {
    if (!blk || !packed_bytes || !nesc) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 nruns = blk->nruns;
    const u64 cap = *packed_bytes;
    *packed_bytes = 0; *nesc = 0;
    if (nruns == 0) return;
    if (!d_packed || !blk->run_count || !blk->run_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (nruns > (u64)TC_MAX_N + 2) TC_FAIL(ctx, TC_ERR_ARG, "too many runs");
    const int fmt = pack_format(blk->sigma);
    if (fmt == 0) {
        if ((uintptr_t)d_packed & 15) TC_FAIL(ctx, TC_ERR_ARG, "packed buffer must be 16-byte aligned");
        const u32 ntiles = tc_cdiv(nruns, PK_TILE);
        u64 *status = nullptr;
        u32 *esc = nullptr;
        // escape scratch: sized for the capacity the caller offers (an escape costs 4 bytes there)
        const u64 esc_cap = cap / 4 < nruns ? cap / 4 : nruns;
        tc_ws_plan(ctx, ws_base, [&](Arena &A, bool) {
            status = A.get<u64>((size_t)ntiles + 2);
            esc = A.get<u32>(esc_cap + 4);
        });
        tc_memset_async(ctx, status, 0, ((size_t)ntiles + 2) * sizeof(u64));
        nib_body_zero(ctx, d_packed, 2 * nruns, cap);     // at most two nibbles per run
        PackNibArgs a;
        a.cnt = blk->run_count; a.val = blk->run_value; a.nruns = nruns;
        a.out = d_packed; a.cap_units = cap / 16;
        a.esc = esc; a.esc_cap = esc_cap;
        a.status = status; a.ticket = reinterpret_cast<u32 *>(status + ntiles); a.err = ctx->d_err;
        a.ntiles = ntiles;
        u32 grid = tc_persistent_grid_for(ctx, pack_nib_kernel, PK_NT, 4);
        if (grid > ntiles) grid = ntiles;
        pack_nib_kernel<<<grid, PK_NT, 0, ctx->stream>>>(a);
        TC_LAUNCH_CHECK(ctx);
        tc_d2h(ctx, &ctx->h_scalars[14], status + (ntiles - 1), sizeof(u64));
        tc_sync_check(ctx);
        const u64 tot = LB_VALUE(ctx->h_scalars[14]);
        const u64 body = (((tot >> NIB_LB_SHIFT) + 31) / 32) * 16, ne = NIB_LB_ESC(tot);
        *nesc = ne;
        *packed_bytes = body + 4 * ne;
        if (*packed_bytes > cap || ne > esc_cap)
            TC_FAIL(ctx, TC_ERR_CAPACITY, "packed runs need %llu bytes", (unsigned long long)*packed_bytes);
        if (ne) {
            TC_HIP(ctx, hipMemcpyAsync(d_packed + body, esc, 4 * ne, hipMemcpyDeviceToDevice, ctx->stream));
            TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return;
    }
    const int bpr = fmt;
    const u64 body = ((u64)bpr * nruns + 7) & ~7ull;
    if (body > cap) {
        *packed_bytes = body;
        TC_FAIL(ctx, TC_ERR_CAPACITY, "packed runs need at least %llu bytes", (unsigned long long)body);
    }
    const u64 esc_cap = (cap - body) / 8;
    u32 *esc = reinterpret_cast<u32 *>(d_packed + body);
    const u32 tiles = tc_cdiv(nruns, PR_TILE);
    u64 *tcnt = nullptr;
    tc_ws_plan(ctx, ws_base, [&](Arena &A, bool) { tcnt = A.get<u64>((size_t)tiles + 2); });
    if (body >= 8) tc_memset_async(ctx, d_packed + body - 8, 0, 8);   // the alignment padding is part of the bytes
    pack_runs_count_kernel<<<tiles, 256, 0, ctx->stream>>>(blk->run_count, nruns, bpr, tcnt);
    TC_LAUNCH_CHECK(ctx);
    scan64_spine_kernel<<<1, 1024, 0, ctx->stream>>>(tcnt, tiles);
    TC_LAUNCH_CHECK(ctx);
    pack_runs_kernel<<<tiles, 256, 0, ctx->stream>>>(blk->run_count, blk->run_value, nruns, bpr, d_packed,
                                                    esc, tcnt, esc_cap);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[14], tcnt + tiles, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *nesc = ctx->h_scalars[14];
    *packed_bytes = body + 8 * *nesc;
    if (*nesc > esc_cap)
        TC_FAIL(ctx, TC_ERR_CAPACITY, "packed runs need %llu bytes", (unsigned long long)*packed_bytes);
}

static void block_unpack_device(tc_ctx *ctx, const uint8_t *d_packed, uint64_t packed_bytes, uint64_t nruns,
                                uint32_t sigma, uint64_t nesc, tc_block *blk) {
    if (!blk || blk->nruns < nruns) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (nruns == 0) { blk->nruns = 0; return; }
    if (!d_packed || !blk->run_count || !blk->run_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const int fmt = pack_format(sigma);
    if (fmt == 0) {
        if ((uintptr_t)d_packed & 15) TC_FAIL(ctx, TC_ERR_ARG, "packed buffer must be 16-byte aligned");
        if (packed_bytes < 4 * nesc || ((packed_bytes - 4 * nesc) & 15) || nesc > nruns)
            TC_FAIL(ctx, TC_ERR_MALFORMED, "packed block: %llu bytes do not hold a nibble body and %llu escapes",
                    (unsigned long long)packed_bytes, (unsigned long long)nesc);
        const u64 body = packed_bytes - 4 * nesc, units = body / 16;
        if (units > (u64)nruns + (nruns + PK_TILE - 1) / PK_TILE + 1)  // > 1 byte per run + padding
            TC_FAIL(ctx, TC_ERR_MALFORMED, "packed block: body too long for %llu runs", (unsigned long long)nruns);
        const u32 ntiles = tc_cdiv(units, UP_TILE_UNITS);
        u64 *status = nullptr;
        tc_ws_plan(ctx, 0, [&](Arena &A, bool) { status = A.get<u64>((size_t)ntiles + 2); });
        tc_memset_async(ctx, status, 0, ((size_t)ntiles + 2) * sizeof(u64));
        UnpackNibArgs a;
        a.body = d_packed; a.units = units;
        a.esc = reinterpret_cast<const u32 *>(d_packed + body); a.nesc = nesc; a.nruns = nruns;
        a.cnt = blk->run_count; a.val = blk->run_value;
        a.status = status; a.ticket = reinterpret_cast<u32 *>(status + ntiles); a.err = ctx->d_err;
        a.ntiles = ntiles;
        u32 grid = tc_persistent_grid_for(ctx, unpack_nib_kernel, UP_NT, 4);
        if (grid > ntiles) grid = ntiles;
        unpack_nib_kernel<<<grid, UP_NT, 0, ctx->stream>>>(a);
        TC_LAUNCH_CHECK(ctx);
        tc_d2h(ctx, &ctx->h_scalars[14], status + (ntiles - 1), sizeof(u64));
        tc_sync_check(ctx);
        const u64 tot = LB_VALUE(ctx->h_scalars[14]);
        if ((tot >> 31) != nruns || (tot & 0x7fffffffull) != nesc)
            TC_FAIL(ctx, TC_ERR_MALFORMED, "packed block holds %llu runs / %llu escapes, header says %llu / %llu",
                    (unsigned long long)(tot >> 31), (unsigned long long)(tot & 0x7fffffffull),
                    (unsigned long long)nruns, (unsigned long long)nesc);
        blk->nruns = nruns;
        blk->sigma = sigma;
        return;
    }
    const int bpr = fmt;
    const u64 body = ((u64)bpr * nruns + 7) & ~7ull;
    if (packed_bytes < body + 8 * nesc) TC_FAIL(ctx, TC_ERR_MALFORMED, "packed block too short");
    u32 grid = tc_cdiv(nruns, 256 * 8);
    if (grid > 8192) grid = 8192;
    unpack_runs_kernel<<<grid, 256, 0, ctx->stream>>>(d_packed, nruns, bpr, blk->run_count, blk->run_value);
    TC_LAUNCH_CHECK(ctx);
    if (nesc) {
        unpack_esc_kernel<<<tc_cdiv(nesc, 256), 256, 0, ctx->stream>>>(
            reinterpret_cast<const u32 *>(d_packed + body), nesc, nruns, blk->run_count);
        TC_LAUNCH_CHECK(ctx);
    }
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    blk->nruns = nruns;
    blk->sigma = sigma;
}

// ====================================================== encoded-block container
// header (TC_CONTAINER_HEADER bytes, little-endian) + packed runs; SURVEY 8f-4
struct ContainerHeader {
    char magic[8];       // "TCBLK01\0"
    u64 n, primary, nruns, nesc, body_bytes, checksum;
    u32 sigma, format;
    i16 final_list[TC_MAX_SIGMA];
};
static_assert(sizeof(ContainerHeader) <= TC_CONTAINER_HEADER, "container header layout");
static const char kContainerMagic[8] = {'T', 'C', 'B', 'L', 'K', '0', '1', 0};

// what a writer knows of the header before the body exists; nruns, nesc, body_bytes and checksum follow the body
static ContainerHeader container_header_host(u64 n, u64 primary, u32 sigma, u32 format, const i16 *final_list) {
    ContainerHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, kContainerMagic, 8);
    h.n = n; h.primary = primary; h.sigma = sigma; h.format = format;
    for (u32 i = 0; i < sigma; i++) h.final_list[i] = final_list[i];
    return h;
}
// the header, zero-padded to TC_CONTAINER_HEADER bytes, to the front of d_out (through the pinned staging, on the stream)
static void container_header_put(tc_ctx *ctx, const ContainerHeader &h, u8 *d_out) {
    memset(ctx->h_hdr, 0, TC_CONTAINER_HEADER);
    memcpy(ctx->h_hdr, &h, sizeof h);
    tc_h2d(ctx, d_out, ctx->h_hdr, TC_CONTAINER_HEADER);
}
// The header at p (host memory, TC_CONTAINER_HEADER bytes; the container has `avail` bytes, header included), checked as
// far as `level` asks -- each level includes the ones before it.
enum HeaderLevel {
    HDR_MAGIC,    // the magic
    HDR_BOUNDS,   // + n and nruns within what the library handles
    HDR_FITS,     // + the body ends inside `avail`
    HDR_FULL      // + every field consistent, the body exactly `avail` long
};
static ContainerHeader container_header_parse(tc_ctx *ctx, const u8 *p, u64 avail, HeaderLevel level) {
    ContainerHeader h;
    memcpy(&h, p, sizeof h);
    if (memcmp(h.magic, kContainerMagic, 8) != 0) TC_FAIL(ctx, TC_ERR_MALFORMED, "not a textcomp container");
    bool bad = false;
    if (level >= HDR_BOUNDS) bad = h.n > TC_MAX_N || h.nruns > (u64)TC_MAX_N + 2;
    if (level >= HDR_FITS) bad = bad || h.body_bytes > avail - TC_CONTAINER_HEADER;
    if (level >= HDR_FULL)
        bad = bad || h.sigma > TC_MAX_SIGMA || h.nesc > h.nruns ||
              (h.format != (u32)pack_format(h.sigma) && !(h.format == HF_FORMAT && h.nesc == 0)) ||
              h.body_bytes != avail - TC_CONTAINER_HEADER || (h.n > 0 && (h.primary > h.n || h.nruns == 0));
    if (bad) TC_FAIL(ctx, TC_ERR_MALFORMED, "container header is inconsistent");
    return h;
}

// the sum a thread of a grid of 256-thread workgroups contributes: word i weighs in by a mix of (word, i); four loads
// in flight per thread (one per loop turn left the memory latency exposed)
__device__ __forceinline__ u64 checksum64_term(u32 word, u64 i) {
    u64 z = ((u64)word << 32 | (u32)i) + (i >> 32) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ u64 checksum64_partial(const u32 *__restrict__ w, u64 nwords) {
    const u64 stride = (u64)gridDim.x * 256;
    u64 i = (u64)blockIdx.x * 256 + threadIdx.x, acc = 0;
    for (; i + 3 * stride < nwords; i += 4 * stride) {
        const u32 a = w[i], b = w[i + stride], c = w[i + 2 * stride], d = w[i + 3 * stride];
        acc += checksum64_term(a, i) + checksum64_term(b, i + stride) + checksum64_term(c, i + 2 * stride) + checksum64_term(d, i + 3 * stride);
    }
    for (; i < nwords; i += stride) acc += checksum64_term(w[i], i);
    return acc;
}
// position-dependent 64-bit checksum of a byte range (16-byte aligned, length a multiple of 4)
// (C linkage, here and for the three seal kernels below: the plain names the profiles list them by)
extern "C" __global__ __launch_bounds__(256) void checksum64_kernel(const u32 *__restrict__ w, u64 nwords, u64 *out) {
    u64 acc = checksum64_partial(w, nwords);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane_id() == 0 && acc) atomicAdd((unsigned long long *)out, (unsigned long long)acc);
}
static u64 checksum64_device(tc_ctx *ctx, const u8 *d_p, u64 bytes) {
    u64 *d_sum = ctx->d_scalars + 16;
    tc_memset_async(ctx, d_sum, 0, sizeof(u64));
    const u64 nwords = bytes / 4;
    if (nwords) {
        u32 grid = tc_cdiv(nwords, 256 * 16);
        if (grid > 4096) grid = 4096;
        checksum64_kernel<<<grid, 256, 0, ctx->stream>>>(reinterpret_cast<const u32 *>(d_p), nwords, d_sum);
        TC_LAUNCH_CHECK(ctx);
    }
    tc_d2h(ctx, &ctx->h_scalars[16], d_sum, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ctx->h_scalars[16] ^ (bytes * 0x9E3779B97F4A7C15ull);
}

// ---- the Huffman body (format 3; tc_huff.hpp, layout in include/textcomp.h) ------------------------------------------
// Writes blk's runs as a Huffman body into d_body (*body_bytes: in capacity, out bytes used) and returns true -- or
// returns false, nothing of value written, when the record is to be packed instead: the Huffman body would not be
// strictly smaller than the packed one (whose size the histogram pass has summed from the counts), or a run has no
// token (count 0, value >= sigma).  Two host synchronisations of its own: the histogram, and the payload size.
static bool huff_write_device(tc_ctx *ctx, const tc_block *blk, u8 *d_body, u64 *body_bytes, size_t ws_base) {
    const u64 nruns = blk->nruns, cap = *body_bytes;
    const u32 sigma = blk->sigma;
    if (nruns == 0 || sigma == 0) return false;
    if (!blk->run_count || !blk->run_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (nruns > (u64)TC_MAX_N + 2) TC_FAIL(ctx, TC_ERR_ARG, "too many runs");
    const u32 nsyms = sigma + 2;
    const u32 nchunks = tc_cdiv(nruns, HF_K);
    u32 *hist = nullptr, *dirbits = nullptr;
    u64 *offs = nullptr;
    tc_ws_plan(ctx, ws_base, [&](Arena &A, bool) {
        hist = A.get<u32>(HF_HIST_WORDS);
        dirbits = A.get<u32>((size_t)nchunks + 4);
        offs = A.get<u64>((size_t)nchunks + 2);
    });
    hipStream_t s = ctx->stream;
    tc_memset_async(ctx, hist, 0, HF_HIST_WORDS * sizeof(u32));
    u32 grid = tc_persistent_grid(ctx, 8);
    {
        HuffHistArgs a;
        a.cnt = blk->run_count; a.val = blk->run_value; a.nruns = nruns; a.sigma = sigma; a.hist = hist;
        const u32 g = tc_cdiv(nruns, HF_NT * 4);
        huff_hist_kernel<<<g < grid ? g : grid, HF_NT, 0, s>>>(a);
        TC_LAUNCH_CHECK(ctx);
    }
    u32 h_hist[HF_HIST_WORDS];
    tc_d2h(ctx, h_hist, hist, sizeof h_hist);
    TC_HIP(ctx, hipStreamSynchronize(s));
    u64 tot[HF_TOT_WORDS / 2];
    memcpy(tot, h_hist + 264, sizeof tot);
    if (tot[4]) return false;   // a run without a token: such a block is packed
    const int fmt = pack_format(sigma);
    const u64 packed = fmt == 0 ? ((tot[0] + 31) / 32) * 16 + 4 * tot[1]
                                : (((u64)fmt * nruns + 7) & ~7ull) + 8 * (fmt == 1 ? tot[2] : tot[3]);
    const u64 fixed = hf_fixed_bytes(nsyms, nchunks);
    if (fixed + 16 >= packed) return false;   // head, lengths and directory alone outweigh the packed body
    u8 len[HF_MAXSYM + 1];
    huff_build_lengths(h_hist, nsyms, len);
    HuffEncArgs e;
    huff_assign_codes(len, nsyms, &e.codes);
    e.cnt = blk->run_count; e.val = blk->run_value; e.nruns = nruns; e.sigma = sigma; e.nchunks = nchunks;
    e.dirbits = dirbits; e.offs = offs; e.payload = nullptr; e.payload_words = 0;
    if (grid > nchunks) grid = nchunks;
    huff_encode_kernel<false><<<grid, HF_NT, 0, s>>>(e);
    TC_LAUNCH_CHECK(ctx);
    huff_dir_scan_kernel<<<1, HF_SCAN_NT, 0, s>>>(dirbits, nchunks, offs);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[14], offs + nchunks, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    const u64 words = ctx->h_scalars[14];
    const u64 body = fixed + hf_pad16(4 * words);
    if (body >= packed) return false;
    *body_bytes = body;
    if (body > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "container body needs %llu bytes", (unsigned long long)body);
    if (!d_body) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    // head and lengths (through the pinned header staging, which is idle until the container's header is written)
    const u64 lens_off = 16, dir_off = 16 + hf_pad16(nsyms), pay_off = fixed;
    u8 *stage = ctx->h_hdr;
    memset(stage, 0, (size_t)dir_off);
    const u32 head[4] = {HF_K, nchunks, nsyms, HF_LMAX};
    memcpy(stage, head, 16);
    memcpy(stage + lens_off, len, nsyms);
    tc_h2d(ctx, d_body, stage, (size_t)dir_off);
    tc_memset_async(ctx, d_body + body - 16, 0, 16);                 // the payload's padding
    tc_memset_async(ctx, d_body + pay_off - 16, 0, 16);             // the directory's padding
    TC_HIP(ctx, hipMemcpyAsync(d_body + dir_off, dirbits, 4 * (size_t)nchunks, hipMemcpyDeviceToDevice, s));
    e.payload = reinterpret_cast<u32 *>(d_body + pay_off);
    e.payload_words = words;
    huff_encode_kernel<true><<<grid, HF_NT, 0, s>>>(e);
    TC_LAUNCH_CHECK(ctx);
    return true;
}

// Inverse: validates head, lengths and directory, then fills blk->run_count / run_value (device, capacity
// blk->nruns >= nruns).  Anything that is not a body of exactly nruns runs is TC_ERR_MALFORMED.
static void huff_read_device(tc_ctx *ctx, const u8 *d_body, u64 body_bytes, u64 nruns, u32 sigma, tc_block *blk) {
    if (!blk || blk->nruns < nruns) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (nruns == 0 || sigma == 0 || sigma > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body without runs");
    if (!d_body || !blk->run_count || !blk->run_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u32 nsyms = sigma + 2;
    const u64 dir_off = 16 + hf_pad16(nsyms);
    if (body_bytes < dir_off || (body_bytes & 15)) TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body too short");
    hipStream_t s = ctx->stream;
    u8 fix[16 + ((HF_MAXSYM + 15) & ~15)];
    tc_d2h(ctx, fix, d_body, (size_t)dir_off);
    TC_HIP(ctx, hipStreamSynchronize(s));
    u32 head[4];
    memcpy(head, fix, 16);
    const u32 K = head[0], nchunks = head[1], lmax = head[3];
    if (K == 0 || (K & (K - 1)) || head[2] != nsyms || lmax < 1 || lmax > HF_LMAX ||
        (u64)nchunks != (nruns + K - 1) / K)
        TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body: bad head (K %u, chunks %u, symbols %u, longest code %u)", K, nchunks,
                head[2], lmax);
    u64 kraft = 0;   // in units of 2^-lmax
    for (u32 i = 0; i < nsyms; i++) {
        const u32 l = fix[16 + i];
        if (l > lmax) TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body: code length %u above %u", l, lmax);
        if (l) kraft += 1ull << (lmax - l);
    }
    if (kraft > (1ull << lmax)) TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body: code lengths are no prefix code");
    const u64 fixed = hf_fixed_bytes(nsyms, nchunks);
    if (fixed > body_bytes) TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body: directory longer than the body");
    const u64 payload_words = (body_bytes - fixed) / 4;
    u64 *offs = nullptr;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) { offs = A.get<u64>((size_t)nchunks + 2); });
    const u32 *dirbits = reinterpret_cast<const u32 *>(d_body + dir_off);
    huff_dir_scan_kernel<<<1, HF_SCAN_NT, 0, s>>>(dirbits, nchunks, offs);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, &ctx->h_scalars[14], offs + nchunks, sizeof(u64));
    TC_HIP(ctx, hipStreamSynchronize(s));
    const u64 words = ctx->h_scalars[14];
    if (((words + 3) & ~3ull) != payload_words)
        TC_FAIL(ctx, TC_ERR_MALFORMED, "Huffman body: directory sums to %llu words, payload has %llu",
                (unsigned long long)words, (unsigned long long)payload_words);
    HuffDecArgs a;
    a.len = d_body + 16; a.dirbits = dirbits; a.offs = offs;
    a.payload = reinterpret_cast<const u32 *>(d_body + fixed); a.payload_words = payload_words;
    a.nruns = nruns; a.K = K; a.nchunks = nchunks; a.sigma = sigma; a.lmax = lmax;
    a.cnt = blk->run_count; a.val = blk->run_value; a.err = ctx->d_err;
    u32 grid = tc_persistent_grid(ctx, 8);
    const u32 g = tc_cdiv(nchunks, HF_NT);
    huff_decode_kernel<<<g < grid ? g : grid, HF_NT, 0, s>>>(a);
    TC_LAUNCH_CHECK(ctx);
    tc_sync_check(ctx);
    blk->nruns = nruns;
    blk->sigma = sigma;
}

static void container_write_device(tc_ctx *ctx, const tc_block *blk, u8 *d_out, u64 *bytes, size_t ws_base = 0) {
    if (!blk || !bytes) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *bytes;
    *bytes = 0;
    if (!d_out || ((uintptr_t)d_out & 15)) TC_FAIL(ctx, TC_ERR_ARG, "container buffer must be 16-byte aligned");
    if (blk->sigma > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_ARG, "bad block");
    if (cap < TC_CONTAINER_HEADER) {
        *bytes = tc_container_bound(blk->nruns, blk->sigma);
        TC_FAIL(ctx, TC_ERR_CAPACITY, "container needs at least %llu bytes", (unsigned long long)*bytes);
    }
    ContainerHeader h = container_header_host(blk->n, blk->primary, blk->sigma, (u32)pack_format(blk->sigma), blk->final_list);
    u64 body = cap - TC_CONTAINER_HEADER, nesc = 0;
    try {
        if (ctx->coding == TC_CODING_HUFFMAN && huff_write_device(ctx, blk, d_out + TC_CONTAINER_HEADER, &body, ws_base)) {
            h.format = HF_FORMAT;
        } else {
            body = cap - TC_CONTAINER_HEADER;
            block_pack_device(ctx, blk, d_out + TC_CONTAINER_HEADER, &body, &nesc, ws_base);
        }
    } catch (const TcFail &f) {
        if (f.code == TC_ERR_CAPACITY) *bytes = TC_CONTAINER_HEADER + body;
        throw;
    }
    h.nruns = blk->nruns; h.nesc = nesc; h.body_bytes = body;
    h.checksum = checksum64_device(ctx, d_out + TC_CONTAINER_HEADER, body);
    container_header_put(ctx, h, d_out);
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *bytes = TC_CONTAINER_HEADER + body;
}

// the header of a container in device memory, fully validated
static ContainerHeader container_header(tc_ctx *ctx, const u8 *d_in, u64 bytes) {
    if (!d_in || ((uintptr_t)d_in & 15)) TC_FAIL(ctx, TC_ERR_ARG, "container buffer must be 16-byte aligned");
    if (bytes < TC_CONTAINER_HEADER) TC_FAIL(ctx, TC_ERR_MALFORMED, "container shorter than its header");
    u8 hdr[TC_CONTAINER_HEADER];
    tc_d2h(ctx, hdr, d_in, TC_CONTAINER_HEADER);
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return container_header_parse(ctx, hdr, bytes, HDR_FULL);
}

static void container_read_device(tc_ctx *ctx, const u8 *d_in, u64 bytes, tc_block *blk) {
    if (!blk) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const ContainerHeader h = container_header(ctx, d_in, bytes);
    if (blk->nruns < h.nruns) {
        blk->nruns = h.nruns;
        TC_FAIL(ctx, TC_ERR_CAPACITY, "block needs %llu run slots", (unsigned long long)h.nruns);
    }
    if (checksum64_device(ctx, d_in + TC_CONTAINER_HEADER, h.body_bytes) != h.checksum)
        TC_FAIL(ctx, TC_ERR_MALFORMED, "container checksum mismatch");
    if (h.format == HF_FORMAT) huff_read_device(ctx, d_in + TC_CONTAINER_HEADER, h.body_bytes, h.nruns, h.sigma, blk);
    else block_unpack_device(ctx, d_in + TC_CONTAINER_HEADER, h.body_bytes, h.nruns, h.sigma, h.nesc, blk);
    blk->n = h.n; blk->primary = h.primary; blk->sigma = h.sigma; blk->nruns = h.nruns;
    for (u32 i = 0; i < h.sigma; i++) blk->final_list[i] = h.final_list[i];
}

// ---- text -> container on the device, the runs never leaving the chip for a small alphabet -----------------
// What the multi-GPU step ships is the container, not the run arrays: for sigma <= 6 (an ACGTN record) the RLE
// stage writes the container's nibble stream itself (rle_nib_kernel, tc_pack.hpp) and three small kernels seal
// the container on the device -- escape list behind the body, checksum, header fields -- so the call has one
// host synchronisation of its own (the sizes it returns).  Larger alphabets take the two-step way (run arrays
// in the workspace, then the byte packers).  The bytes are those of tc_encode_dev + tc_block_to_container_dev.
extern "C" __global__ __launch_bounds__(256) void nib_escapes_kernel(const u64 *__restrict__ totals, const u32 *__restrict__ esc,
                                                          u8 *__restrict__ body, u64 cap_bytes, u64 esc_cap) {
    const u64 units = (totals[1] + 31) >> 5;
    u64 nesc = totals[2];
    if (nesc > esc_cap) nesc = esc_cap;
    u32 *dst = reinterpret_cast<u32 *>(body + 16 * units);
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < nesc; i += (u64)gridDim.x * 256)
        if (16 * units + 4 * (i + 1) <= cap_bytes) dst[i] = esc[i];
}
// checksum64_kernel over a body whose length is known on the device only
extern "C" __global__ __launch_bounds__(256) void checksum64_dyn_kernel(const u32 *__restrict__ w, const u64 *__restrict__ totals,
                                                             u64 cap_bytes, u64 *out) {
    u64 nwords = 4 * ((totals[1] + 31) >> 5) + totals[2];
    if (nwords > cap_bytes / 4) nwords = cap_bytes / 4;
    u64 acc = checksum64_partial(w, nwords);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane_id() == 0 && acc) atomicAdd((unsigned long long *)out, (unsigned long long)acc);
}
// header fields that only the device knows: nruns @24, nesc @32, body_bytes @40, checksum @48 (ContainerHeader)
extern "C" __global__ void container_seal_kernel(u8 *hdr, const u64 *totals, const u64 *sum, u64 *result) {
    const u64 nruns = totals[0], nesc = totals[2], body = 16 * ((totals[1] + 31) >> 5) + 4 * nesc;
    u64 *h = reinterpret_cast<u64 *>(hdr);
    h[3] = nruns; h[4] = nesc; h[5] = body;
    h[6] = *sum ^ (body * 0x9E3779B97F4A7C15ull);
    result[0] = nruns; result[1] = nesc; result[2] = body;
}

static void encode_container_device(tc_ctx *ctx, const u8 *d_text, u64 n, u8 *d_out, u64 *bytes) {
    const u64 cap = *bytes;
    *bytes = 0;
    if (!d_out || ((uintptr_t)d_out & 15)) TC_FAIL(ctx, TC_ERR_ARG, "container buffer must be 16-byte aligned");
    if (cap < TC_CONTAINER_HEADER) {
        *bytes = tc_container_bound(n + 2, TC_MAX_SIGMA);
        TC_FAIL(ctx, TC_ERR_CAPACITY, "container needs at least %d bytes", TC_CONTAINER_HEADER);
    }
    if (n == 0) {   // empty in, empty out: a header with no runs
        tc_block e;
        memset(&e, 0, sizeof e);
        *bytes = cap;
        container_write_device(ctx, &e, d_out, bytes, 0);
        return;
    }
    const u64 N = n + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    u64 primary = 0;
    u32 counts257[257];
    u32 sigma = 0;
    i16 final_list[TC_MAX_SIGMA];
    hipStream_t s = ctx->stream;
    static_assert(RN_TILE == MTF_TILE, "one tile count for the nibble-stream kernels");
    const u32 ntiles = tc_cdiv(N, RN_TILE);
    const size_t status_words = 2 * (size_t)ntiles + 32;
    const u64 esc_cap = N / 5 + 16;
    u8 *const body = d_out + TC_CONTAINER_HEADER;
    const u64 body_cap = cap - TC_CONTAINER_HEADER;
    bool fused = false;
    // a Huffman-coded container is written from the run arrays (as sigma > 6 is): neither fused nibble path is taken
    const bool huff = ctx->coding == TC_CODING_HUFFMAN;
    tc_block blk;
    memset(&blk, 0, sizeof blk);
    size_t pack_base = 0;
    // what both fused paths do around their kernel: the status words and the body start out zero (at most one nibble
    // per symbol) ...
    auto zero = [&](u64 *status) {
        tc_memset_async(ctx, status, 0, status_words * sizeof(u64));
        nib_body_zero(ctx, body, N, body_cap);
    };
    // ... what the host knows of the header goes in front ...
    auto write_header = [&]() {
        container_header_put(ctx, container_header_host(n, primary, sigma, (u32)pack_format(sigma), final_list), d_out);
    };
    // ... and the seal kernels fill in the rest, on the device: the call's one host synchronisation reads their result
    auto seal = [&](u64 *totals, u32 *esc_list) {
        u64 *sum = totals + 4, *result = totals + 5;
        nib_escapes_kernel<<<64, 256, 0, s>>>(totals, esc_list, body, body_cap, esc_cap);
        TC_LAUNCH_CHECK(ctx);
        checksum64_dyn_kernel<<<4096, 256, 0, s>>>(reinterpret_cast<const u32 *>(body), totals, body_cap, sum);
        TC_LAUNCH_CHECK(ctx);
        container_seal_kernel<<<1, 1, 0, s>>>(d_out, totals, sum, result);
        TC_LAUNCH_CHECK(ctx);
        TC_HIP(ctx, hipEventRecord(ctx->ev[3], s));
        tc_d2h(ctx, &ctx->h_scalars[20], result, 3 * sizeof(u64));
    };
    tc_ws_plan(ctx, 0, [&](Arena &A, bool dry) {
        u16 *d_idx = nullptr;
        BwtAcc acc = encode_sa_stage(ctx, A, dry, d_text, n, 16, &d_idx, &primary, counts257);
        bool idx8 = false;
        // a record over <= 6 symbols: MTF, RLE and the wire format in ONE kernel (tc_pack.hpp, mtf_rle_kernel<true>);
        // its scratch first (the dry run does not know sigma yet)
        u64 *fstatus = A.get<u64>(status_words);
        u32 *fesc = A.get<u32>(esc_cap);
        bool one_kernel = false;
        if (!dry && !huff && env_int("TC_MTF_RLE", 1) != 0 && env_int("TC_MTF_FORCE_GENERAL", 0) == 0 && N + 64 < (1ull << 32)) {
            Alphabet al;
            al.build(counts257);
            if (al.sigma <= PK_NIB_SIGMA) {
                zero(fstatus);
                MtfRleArgs a;
                memset(&a, 0, sizeof a);
                for (int v = 0; v < 257; v++) a.lut.v[v] = (u8)al.code_of_sym[v];
                a.acc = acc; a.N = N; a.sigma = al.sigma;
                a.status_a = fstatus; a.status_b = fstatus + ntiles;
                a.ticket = reinterpret_cast<u32 *>(fstatus + 2 * (size_t)ntiles);
                a.flag = reinterpret_cast<u32 *>(fstatus + 2 * (size_t)ntiles + 1);
                a.totals = fstatus + 2 * (size_t)ntiles + 8;
                a.scalars = ctx->d_scalars; a.err = ctx->d_err; a.ntiles = ntiles;
                a.out = body; a.cap_units = body_cap / 16; a.esc = fesc; a.esc_cap = esc_cap;
                mtf_rle_kernel<true><<<ntiles, MTF_NT, 0, s>>>(a);
                TC_LAUNCH_CHECK(ctx);
                u64 *d_final = fstatus + 2 * (size_t)ntiles + 2;
                mtf_nib_final_kernel<BwtAcc><<<1, 64, 0, s>>>(acc, N, a.lut, al.sigma, d_final, a.flag);
                TC_LAUNCH_CHECK(ctx);
                tc_d2h(ctx, &ctx->h_scalars[15], a.flag, sizeof(u32));
                tc_d2h(ctx, &ctx->h_scalars[8], d_final, sizeof(u64));
                TC_HIP(ctx, hipStreamSynchronize(s));
                if ((u32)ctx->h_scalars[15] == 0) {
                    const u64 perm = ctx->h_scalars[8];
                    sigma = al.sigma;
                    for (u32 i = 0; i < sigma; i++) final_list[i] = al.sym_of_code[(perm >> (4 * i)) & 15];
                    TC_HIP(ctx, hipEventRecord(ctx->ev[2], s));
                    write_header();
                    seal(a.totals, fesc);
                    one_kernel = true;
                    fused = true;
                } else {
                    ctx->mtf_fastin_failed = 1;
                }
            }
        }
        if (!one_kernel) {
            mtf_encode_device<BwtAcc>(ctx, A, acc, N, dry ? nullptr : counts257, d_idx, final_list, &sigma, dry,
                                      reinterpret_cast<u8 *>(d_idx), &idx8);
            if (!dry) TC_HIP(ctx, hipEventRecord(ctx->ev[2], s));
        }
        // scratch of both ways (the dry run does not know sigma yet)
        u64 *status = A.get<u64>(status_words);
        u32 *esc = A.get<u32>(esc_cap);
        u32 *r_cnt = A.get<u32>(N + 2);
        u16 *r_val = A.get<u16>(N + 2);
        size_t rle_mark = A.off;
        if (dry) {
            U16Acc iacc{d_idx};
            u64 t = 0;
            rle_encode_device<U16Acc, u16>(ctx, A, iacc, N, r_cnt, r_val, N + 2, &t, true);
            pack_base = A.off;
            (void)A.get<u8>(container_scratch(ctx, N + 2));
        } else if (!one_kernel && idx8 && sigma <= PK_NIB_SIGMA && !huff) {   // the byte-wide index stream into the nibble stream
            fused = true;
            zero(status);
            write_header();
            RleNibArgs a;
            a.src = reinterpret_cast<const u8 *>(d_idx); a.N = N;
            a.out = body; a.cap_units = body_cap / 16;
            a.esc = esc; a.esc_cap = esc_cap;
            a.status_a = status; a.status_b = status + ntiles;
            a.ticket = reinterpret_cast<u32 *>(status + 2 * (size_t)ntiles);
            a.totals = status + 2 * (size_t)ntiles + 8;
            a.err = ctx->d_err; a.ntiles = ntiles;
            a.diag = env_int("TC_RLE_DIAG", 0);
            u32 grid = tc_persistent_grid_for(ctx, rle_nib_kernel, RN_NT, 8);
            if (grid > ntiles) grid = ntiles;
            rle_nib_kernel<<<grid, RN_NT, 0, s>>>(a);
            TC_LAUNCH_CHECK(ctx);
            seal(a.totals, esc);
        } else if (!one_kernel) {   // the run arrays, for the packers or the Huffman writer
            u64 total = 0;
            A.rewind(rle_mark);
            if (idx8) {
                U8Acc iacc{reinterpret_cast<const u8 *>(d_idx)};
                rle_encode_device<U8Acc, u16>(ctx, A, iacc, N, r_cnt, r_val, N + 2, &total, false, sigma <= 16);
            } else {
                U16Acc iacc{d_idx};
                rle_encode_device<U16Acc, u16>(ctx, A, iacc, N, r_cnt, r_val, N + 2, &total, false);
            }
            TC_HIP(ctx, hipEventRecord(ctx->ev[3], s));
            blk.n = n; blk.primary = primary; blk.sigma = sigma; blk.nruns = total;
            blk.run_count = r_cnt; blk.run_value = r_val;
            for (u32 i = 0; i < sigma; i++) blk.final_list[i] = final_list[i];
        }
    });
    tc_sync_check(ctx);
    encode_stage_times(ctx);
    if (fused) {
        const u64 nruns = ctx->h_scalars[20], nesc = ctx->h_scalars[21], body_bytes = ctx->h_scalars[22];
        ctx->stats.runs = nruns;
        *bytes = TC_CONTAINER_HEADER + body_bytes;
        if (*bytes > cap || nesc > esc_cap)
            TC_FAIL(ctx, TC_ERR_CAPACITY, "container needs %llu bytes", (unsigned long long)*bytes);
        return;
    }
    ctx->stats.runs = blk.nruns;
    *bytes = cap;
    container_write_device(ctx, &blk, d_out, bytes, pack_base);
}

// ---- the chunked stream as a wire format: the bound of a record's container and the walk over a stream's headers
// (its two-slot pipeline: tc_hostio_host.hpp) ----------------------------------------------------------------------
// room for the container of an n-byte record, whatever its alphabet
static u64 container_bound_any(u64 n) {
    u64 b = 0;
    for (u32 sg : {6u, 16u, 257u}) {
        const u64 v = tc_container_bound(n + 2, sg);
        if (v > b) b = v;
    }
    return b;
}

// walks the containers of a stream in HOST memory: offsets, total text length, largest record
struct StreamIndex {
    std::vector<u64> off, len, n, nruns;
    u64 n_total = 0, n_max = 0, len_max = 0, nruns_max = 0;
};
static StreamIndex stream_index(tc_ctx *ctx, const u8 *stream, u64 bytes) {
    StreamIndex ix;
    if (!stream || bytes < TC_CONTAINER_HEADER) TC_FAIL(ctx, TC_ERR_MALFORMED, "stream shorter than one container header");
    u64 off = 0;
    while (off < bytes) {
        if (bytes - off < TC_CONTAINER_HEADER) TC_FAIL(ctx, TC_ERR_MALFORMED, "stream ends inside a container header");
        const ContainerHeader h = container_header_parse(ctx, stream + off, bytes - off, HDR_FITS);
        const u64 len = TC_CONTAINER_HEADER + h.body_bytes;
        ix.off.push_back(off); ix.len.push_back(len); ix.n.push_back(h.n); ix.nruns.push_back(h.nruns);
        ix.n_total += h.n;
        if (h.n > ix.n_max) ix.n_max = h.n;
        if (len > ix.len_max) ix.len_max = len;
        if (h.nruns > ix.nruns_max) ix.nruns_max = h.nruns;
        off += len;
    }
    return ix;
}
