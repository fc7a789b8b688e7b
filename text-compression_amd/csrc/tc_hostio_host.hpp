// tc_hostio_host.hpp -- what the entry points that take HOST buffers stand on, and their bodies: the single-stage calls
// (tc_bwt_*, tc_mtf_*, tc_rle_*: upload, run, download through the workspace), the staged copy ring and the persistent
// device buffers of tc_encode / tc_*_container (HostPipe), the owner of what one call allocates (CallScope), and the
// two-slot pipeline of the chunked stream.  The device-pointer forms of these calls check their arguments here too,
// beside the host form.  Included by textcomp.hip only, after tc_ws_host.hpp.
#pragma once
#include <thread>
#include <vector>

#include "tc_container_host.hpp"
#include "tc_decode_host.hpp"

// ================================================================ single stages
// host-pointer form: stage H2D, run, stage D2H
static void bwt_host(tc_ctx *ctx, const u8 *text, u64 n, u8 *L, u32 *sa, u64 *primary) {
    const u64 N = n + 1;
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = N;
    auto plan = [&](Arena &A, bool dry, u8 *&d_text, u8 *&d_L, u32 *&d_sa) {
        d_text = A.get<u8>(n + 16);
        d_L = A.get<u8>(N + 16);
        d_sa = sa ? A.get<u32>(N) : nullptr;    // (no suffix array asked for: the sort may move keys only)
        sa_build(ctx, A, d_text, n, d_sa, d_L, primary, nullptr, dry);
    };
    u8 *d_text, *d_L;
    u32 *d_sa;
    Arena dry(nullptr);
    plan(dry, true, d_text, d_L, d_sa);
    tc_ws_reserve(ctx, dry.peak);
    // carve input first, upload, then run (the upload between the reserve and the run is why this is no tc_ws_plan)
    {
        Arena A0(ctx->ws);
        u8 *t = A0.get<u8>(n + 16);
        tc_h2d(ctx, t, text, n);
    }
    Arena A(ctx->ws);
    plan(A, false, d_text, d_L, d_sa);
    if (L) tc_d2h(ctx, L, d_L, N);
    if (sa) tc_d2h(ctx, sa, d_sa, N * sizeof(u32));
    tc_sync_check(ctx);
}

template <class Acc>
static void mtf_host(tc_ctx *ctx, const void *src, size_t src_bytes, u64 N,
                     i64 primary, u16 *idx, i16 *final_list, u32 *sigma) {
    u8 *d_src = nullptr;
    u16 *d_idx = nullptr;
    auto plan = [&](Arena &A, bool dry) {
        d_src = A.get<u8>(src_bytes + 16);
        d_idx = A.get<u16>(N);
        if (!dry) tc_h2d(ctx, d_src, src, src_bytes);
        Acc acc = make_acc<Acc>(d_src, primary);
        mtf_encode_device<Acc>(ctx, A, acc, N, nullptr, d_idx, final_list, sigma, dry);
    };
    tc_ws_plan(ctx, 0, plan);
    tc_d2h(ctx, idx, d_idx, N * sizeof(u16));
    tc_sync_check(ctx);
}

template <class Acc, class SymT>
static void rle_host(tc_ctx *ctx, const void *src, size_t src_bytes, u64 N, i64 primary,
                     u32 *counts, SymT *syms, u64 *nruns) {
    const u64 cap = *nruns;
    u8 *d_src = nullptr;
    u32 *d_counts = nullptr;
    SymT *d_syms = nullptr;
    u64 total = 0;
    auto plan = [&](Arena &A, bool dry) {
        d_src = A.get<u8>(src_bytes + 16);
        d_counts = A.get<u32>(cap + 1);
        d_syms = A.get<SymT>(cap + 1);
        if (!dry) tc_h2d(ctx, d_src, src, src_bytes);
        Acc acc = make_acc<Acc>(d_src, primary);
        rle_encode_device<Acc, SymT>(ctx, A, acc, N, d_counts, d_syms, cap, &total, dry);
    };
    tc_ws_plan(ctx, 0, plan);
    *nruns = total;
    if (total > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu run slots, have %llu",
                             (unsigned long long)total, (unsigned long long)cap);
    tc_d2h(ctx, counts, d_counts, total * sizeof(u32));
    tc_d2h(ctx, syms, d_syms, total * sizeof(SymT));
    tc_sync_check(ctx);
}

// ------------------------------------------------------------ decode helpers
template <class Acc>
static void ibwt_host(tc_ctx *ctx, const void *src, size_t src_bytes, u64 N, i64 primary, u8 *text,
                      u64 *n_out) {
    u8 *d_src = nullptr, *d_text = nullptr;
    auto plan = [&](Arena &A, bool dry) {
        d_src = A.get<u8>(src_bytes + 16);
        d_text = A.get<u8>(N + 16);
        if (!dry) tc_h2d(ctx, d_src, src, src_bytes);
        Acc acc = make_acc<Acc>(d_src, primary);
        ibwt_device<Acc>(ctx, A, acc, N, nullptr, d_text, n_out, dry);
    };
    tc_ws_plan(ctx, 0, plan);
    tc_sync_check(ctx);
    if (*n_out) {
        tc_d2h(ctx, text, d_text, *n_out);
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
}

template <class SymT>
static void rle_decode_host(tc_ctx *ctx, const u32 *counts, const SymT *syms, u64 nruns,
                            bool has_nothing, SymT *out, u64 *N) {
    const u64 cap = *N;
    u32 *d_counts = nullptr;
    SymT *d_syms = nullptr, *d_out = nullptr;
    u64 total = 0;
    auto plan = [&](Arena &A, bool dry) {
        d_counts = A.get<u32>(nruns + 1);
        d_syms = A.get<SymT>(nruns + 1);
        d_out = A.get<SymT>(cap + 1);
        if (!dry) {
            tc_h2d(ctx, d_counts, counts, nruns * sizeof(u32));
            tc_h2d(ctx, d_syms, syms, nruns * sizeof(SymT));
        }
        rle_decode_device<SymT>(ctx, A, d_counts, d_syms, nruns, has_nothing, d_out, cap, &total, dry);
    };
    tc_ws_plan(ctx, 0, plan);
    *N = total;
    if (total > cap) TC_FAIL(ctx, TC_ERR_CAPACITY, "need %llu output slots, have %llu",
                             (unsigned long long)total, (unsigned long long)cap);
    if (total) tc_d2h(ctx, out, d_out, total * sizeof(SymT));
    tc_sync_check(ctx);
}

// ---- the bodies of the single-stage entry points: Data.BWT
// tc_bwt_encode, and tc_bwt_encode_dev (on_dev: the text and the last column are device memory)
static void bwt_encode_entry(tc_ctx *ctx, const u8 *text, u64 n, u8 *L, u64 *primary, bool on_dev) {
    if (n > TC_MAX_N || !primary) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) { *primary = 0; return; }  // BWT.hs:58
    if (!text || !L) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (!on_dev) return bwt_host(ctx, text, n, L, nullptr, primary);
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = n + 1;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool dry) { sa_build(ctx, A, text, n, nullptr, L, primary, nullptr, dry); });
    tc_sync_check(ctx);
}
static void suffix_array_entry(tc_ctx *ctx, const u8 *text, u64 n, u32 *sa) {
    if (n > TC_MAX_N || !sa) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) { sa[0] = 0; return; }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u64 primary;
    bwt_host(ctx, text, n, nullptr, sa, &primary);
}
static void bwt_decode_entry(tc_ctx *ctx, const u8 *L, u64 N, u64 primary, u8 *text) {
    if (N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) return;
    if (!L || !text || primary >= N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    u64 n_out = 0;
    ibwt_host<BwtAcc>(ctx, L, N, N, (i64)primary, text, &n_out);
    if (n_out != N - 1) TC_FAIL(ctx, TC_ERR_ARG, "not the BWT of any text (cycle of %llu rows)",
                                (unsigned long long)(n_out + 1));
}
static void bwt_decode_sym_entry(tc_ctx *ctx, const i16 *sym, u64 N, u8 *text, u64 *n_out) {
    if (!n_out || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    *n_out = 0;
    if (N == 0) return;  // BWT/Internal.hs:164-167
    if (!sym || !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    ibwt_host<SymAcc>(ctx, sym, N * sizeof(i16), N, -1, text, n_out);
}

// ---- Data.MTF
static void mtf_encode_entry(tc_ctx *ctx, const u8 *L, u64 N, i64 primary, u16 *idx, i16 *final_list, u32 *sigma) {
    if (!sigma || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *sigma = 0; return; }  // MTF/Internal.hs:129-132
    if (!L || !idx || !final_list || primary >= (i64)N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    mtf_host<BwtAcc>(ctx, L, N, N, primary < 0 ? -1 : primary, idx, final_list, sigma);
}
static void mtf_encode_sym_entry(tc_ctx *ctx, const i16 *sym, u64 N, u16 *idx, i16 *final_list, u32 *sigma) {
    if (!sigma || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *sigma = 0; return; }
    if (!sym || !idx || !final_list) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    mtf_host<SymAcc>(ctx, sym, N * sizeof(i16), N, -1, idx, final_list, sigma);
}
static void mtf_decode_entry(tc_ctx *ctx, const u16 *idx, u64 N, const i16 *list, u32 nlist, i16 *sym) {
    if (N > TC_MAX_N + 1 || nlist > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0 || nlist == 0) return;  // MTF/Internal.hs:202-209
    if (!idx || !list || !sym) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u16 *d_idx = nullptr;
    i16 *d_sym = nullptr;
    auto plan = [&](Arena &A, bool dry) {
        d_idx = A.get<u16>(N + 64);
        d_sym = A.get<i16>(N + 64);
        if (!dry) tc_h2d(ctx, d_idx, idx, N * sizeof(u16));
        mtf_decode_device(ctx, A, d_idx, N, list, nlist, d_sym, dry);
    };
    tc_ws_plan(ctx, 0, plan);
    tc_d2h(ctx, sym, d_sym, N * sizeof(i16));
    tc_sync_check(ctx);
}

// ---- Data.RLE
static void rle_encode_entry(tc_ctx *ctx, const u8 *L, u64 N, i64 primary, u32 *counts, i16 *syms, u64 *nruns) {
    if (!nruns || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *nruns = 0; return; }  // RLE.hs:119
    if (!L || !counts || !syms || primary >= (i64)N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    rle_host<BwtAcc, i16>(ctx, L, N, N, primary < 0 ? -1 : primary, counts, syms, nruns);
}
// tc_rle_encode_sym (SymAcc, i16; RLE.hs:157) and tc_rle_encode_u16 (U16Acc, u16)
template <class Acc, class SymT>
static void rle_encode_vals_entry(tc_ctx *ctx, const SymT *vals, u64 N, u32 *counts, SymT *run_vals, u64 *nruns) {
    if (!nruns || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *nruns = 0; return; }
    if (!vals || !counts || !run_vals) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    rle_host<Acc, SymT>(ctx, vals, N * sizeof(SymT), N, -1, counts, run_vals, nruns);
}
// tc_rle_decode (SymT = i16; RLE/Internal.hs:156-159) and tc_rle_decode_u16
template <class SymT>
static void rle_decode_entry(tc_ctx *ctx, const u32 *counts, const SymT *syms, u64 nruns, SymT *out, u64 *N) {
    if (!N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (nruns == 0) { *N = 0; return; }
    if (!counts || !syms || (!out && *N)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    rle_decode_host<SymT>(ctx, counts, syms, nruns, std::is_same<SymT, i16>::value, out, N);
}

// ================================================== host buffers in and out (the path every Haskell caller takes)
// bytestringToBWT and friends hand over a host ByteString (reference BWT.hs:68-70, RLE.hs:83-85).  Until round 3 the
// host entry points paid a hipMalloc / hipFree per buffer per call and one blocking copy of a pageable buffer each
// way (0.95 GB/s for the 1 GiB record).  Now a context keeps (i) its device-side text / output buffers between calls
// (grown, never shrunk) and (ii) a ring of page-locked staging buffers with HP_WORKERS helper threads: a pageable
// buffer crosses in HP_CHUNK pieces -- each worker copies its piece into its staging buffer and posts the DMA on its own
// stream, so the host's memcpy of one piece runs beside the DMA of the others (both directions).  A buffer the caller
// has page-locked itself (hipHostMalloc / hipHostRegister) is recognised and goes by one asynchronous copy.
#define HP_WORKERS 4
#define HP_CHUNK ((size_t)16 << 20)
struct HostPipe {
    u8 *pin[HP_WORKERS][2] = {};
    hipStream_t st[HP_WORKERS] = {};
    hipEvent_t ev[HP_WORKERS][2] = {};
    u8 *d_buf[4] = {};        // persistent device buffers: 0 text / container in, 1 container / text out, 2 run counts, 3 run values
    size_t d_cap[4] = {};
};
static void hp_destroy(HostPipe *hp) {
    for (int w = 0; w < HP_WORKERS; w++) {
        if (hp->st[w]) (void)hipStreamSynchronize(hp->st[w]);
        for (int q = 0; q < 2; q++) {
            if (hp->pin[w][q]) (void)hipHostFree(hp->pin[w][q]);
            if (hp->ev[w][q]) (void)hipEventDestroy(hp->ev[w][q]);
        }
        if (hp->st[w]) (void)hipStreamDestroy(hp->st[w]);
    }
    for (int i = 0; i < 4; i++)
        if (hp->d_buf[i]) (void)hipFree(hp->d_buf[i]);
    delete hp;
}
static HostPipe *hp_get(tc_ctx *ctx) {
    if (ctx->hostpipe) return static_cast<HostPipe *>(ctx->hostpipe);
    // attached only once complete: a failed allocation leaves the context without a pipe (the next
    // call builds one again), never with a half-built one whose null streams and buffers get used
    HostPipe *hp = new HostPipe();
    try {
        for (int w = 0; w < HP_WORKERS; w++) {
            TC_HIP(ctx, hipStreamCreateWithFlags(&hp->st[w], hipStreamNonBlocking));
            for (int q = 0; q < 2; q++) {
                TC_HIP(ctx, hipHostMalloc((void **)&hp->pin[w][q], HP_CHUNK, hipHostMallocDefault));
                TC_HIP(ctx, hipEventCreateWithFlags(&hp->ev[w][q], hipEventDisableTiming));
            }
        }
    } catch (...) {
        hp_destroy(hp);
        throw;
    }
    ctx->hostpipe = hp;
    return hp;
}
static void hp_release(tc_ctx *ctx) {
    HostPipe *hp = static_cast<HostPipe *>(ctx->hostpipe);
    if (!hp) return;
    hp_destroy(hp);
    ctx->hostpipe = nullptr;
}
// persistent device buffer `which` of at least `bytes` (kept across calls; a longer request replaces it)
static u8 *hp_dev(tc_ctx *ctx, int which, size_t bytes) {
    HostPipe *hp = hp_get(ctx);
    if (hp->d_cap[which] >= bytes && hp->d_buf[which]) return hp->d_buf[which];
    if (hp->d_buf[which]) {
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(hp->d_buf[which]);
        hp->d_buf[which] = nullptr; hp->d_cap[which] = 0;
    }
    const size_t want = (bytes + (bytes >> 5) + ((size_t)2 << 20)) & ~(((size_t)2 << 20) - 1);
    if (hipMalloc((void **)&hp->d_buf[which], want) != hipSuccess) {
        (void)hipGetLastError();
        TC_HIP(ctx, hipMalloc((void **)&hp->d_buf[which], bytes + 256));
        hp->d_cap[which] = bytes + 256;
    } else {
        hp->d_cap[which] = want;
    }
    return hp->d_buf[which];
}
static bool hp_page_locked(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
// host -> device (to_dev) or device -> host, `bytes` bytes; returns when the data has arrived.  The device side must be
// complete on the context's stream before a device -> host copy is asked for (the callers have synchronised).
static void hp_copy(tc_ctx *ctx, void *dst, const void *src, size_t bytes, bool to_dev) {
    if (!bytes) return;
    const void *host = to_dev ? src : dst;
    if (bytes < (1u << 20) || hp_page_locked(host) || env_int("TC_HOST_STAGED", 1) == 0) {
        TC_HIP(ctx, hipMemcpyAsync(dst, src, bytes, to_dev ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return;
    }
    HostPipe *hp = hp_get(ctx);
    const size_t nch = (bytes + HP_CHUNK - 1) / HP_CHUNK;
    hipError_t errs[HP_WORKERS];
    std::thread th[HP_WORKERS];
    const int device = ctx->device;
    for (int w = 0; w < HP_WORKERS; w++) {
        errs[w] = hipSuccess;
        th[w] = std::thread([=, &errs] {
            hipError_t e = hipSetDevice(device);
            auto len_of = [&](size_t c) { return c * HP_CHUNK + HP_CHUNK <= bytes ? HP_CHUNK : bytes - c * HP_CHUNK; };
            if (to_dev) {
                int q = 0;
                bool used[2] = {false, false};
                for (size_t c = (size_t)w; c < nch && e == hipSuccess; c += HP_WORKERS, q ^= 1) {
                    if (used[q]) e = hipEventSynchronize(hp->ev[w][q]);      // the DMA that last read this staging buffer
                    if (e != hipSuccess) break;
                    memcpy(hp->pin[w][q], (const u8 *)src + c * HP_CHUNK, len_of(c));
                    e = hipMemcpyAsync((u8 *)dst + c * HP_CHUNK, hp->pin[w][q], len_of(c), hipMemcpyHostToDevice, hp->st[w]);
                    if (e == hipSuccess) e = hipEventRecord(hp->ev[w][q], hp->st[w]);
                    used[q] = true;
                }
                if (e == hipSuccess) e = hipStreamSynchronize(hp->st[w]);
            } else {
                // the DMA of piece c + WORKERS runs while piece c is copied out of its staging buffer
                int q = 0;
                size_t c = (size_t)w;
                if (c < nch) {
                    e = hipMemcpyAsync(hp->pin[w][q], (const u8 *)src + c * HP_CHUNK, len_of(c), hipMemcpyDeviceToHost, hp->st[w]);
                    if (e == hipSuccess) e = hipEventRecord(hp->ev[w][q], hp->st[w]);
                }
                for (; c < nch && e == hipSuccess; c += HP_WORKERS, q ^= 1) {
                    const size_t nx = c + HP_WORKERS;
                    if (nx < nch) {
                        e = hipMemcpyAsync(hp->pin[w][q ^ 1], (const u8 *)src + nx * HP_CHUNK, len_of(nx), hipMemcpyDeviceToHost, hp->st[w]);
                        if (e == hipSuccess) e = hipEventRecord(hp->ev[w][q ^ 1], hp->st[w]);
                        if (e != hipSuccess) break;
                    }
                    e = hipEventSynchronize(hp->ev[w][q]);
                    if (e != hipSuccess) break;
                    memcpy((u8 *)dst + c * HP_CHUNK, hp->pin[w][q], len_of(c));
                }
                if (e == hipSuccess) e = hipStreamSynchronize(hp->st[w]);
            }
            errs[w] = e;
        });
    }
    hipError_t bad = hipSuccess;
    for (int w = 0; w < HP_WORKERS; w++) {
        th[w].join();
        if (errs[w] != hipSuccess) bad = errs[w];
    }
    if (bad != hipSuccess) {
        (void)hipGetLastError();
        TC_HIP(ctx, bad);
    }
}

// What ONE call allocates on the device beside the context's own buffers: its buffers and streams, given back when
// the call leaves, by return or by any exception.  Declare a CopyJob after its scope: the job is then joined first,
// and the order on the way out is join, wait for the context's stream, free, destroy the streams.
struct CallScope {
    tc_ctx *ctx;
    std::vector<void *> bufs;
    std::vector<hipStream_t> streams;
    explicit CallScope(tc_ctx *c) : ctx(c) {}
    CallScope(const CallScope &) = delete;
    template <class T> T *dev(size_t count) {
        bufs.reserve(bufs.size() + 1);   // (so that nothing throws between the allocation and its entry)
        void *p = nullptr;
        TC_HIP(ctx, hipMalloc(&p, count * sizeof(T)));
        bufs.push_back(p);
        return static_cast<T *>(p);
    }
    hipStream_t stream() {
        streams.reserve(streams.size() + 1);
        hipStream_t s = nullptr;
        TC_HIP(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        streams.push_back(s);
        return s;
    }
    ~CallScope() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : bufs) (void)hipFree(p);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    }
};

// ---- the fused pipeline: tc_encode_dev / tc_encode, tc_decode_dev / tc_decode
// (on_dev: the text and the block's run arrays are device memory)
static void encode_entry(tc_ctx *ctx, const u8 *text, u64 n, tc_block *out, bool on_dev) {
    if (!out || n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = out->nruns;
    u32 *h_count = out->run_count;
    u16 *h_value = out->run_value;
    out->n = n; out->primary = 0; out->sigma = 0; out->nruns = 0;
    if (n == 0) {              // empty in, empty out (BWT.hs:58, MTF.hs:157, RLE.hs:119)
        ctx->stats = tc_stats{};   // (the stats describe this call alone: encode_device resets them otherwise)
        return;
    }
    if (!text || !h_count || !h_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (on_dev) return encode_device(ctx, text, n, out, cap);
    // the device-side buffers live outside the workspace (the pipeline re-carves it) and stay with the context
    u8 *d_text = hp_dev(ctx, 0, n + 16);
    u32 *d_count = reinterpret_cast<u32 *>(hp_dev(ctx, 2, (cap + 1) * sizeof(u32)));
    u16 *d_value = reinterpret_cast<u16 *>(hp_dev(ctx, 3, (cap + 1) * sizeof(u16)));
    hp_copy(ctx, d_text, text, n, true);
    tc_block dev = *out;
    dev.nruns = cap; dev.run_count = d_count; dev.run_value = d_value;
    encode_device(ctx, d_text, n, &dev, cap);
    *out = dev;
    out->run_count = h_count; out->run_value = h_value;
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hp_copy(ctx, h_count, d_count, dev.nruns * sizeof(u32), false);
    hp_copy(ctx, h_value, d_value, dev.nruns * sizeof(u16), false);
}
static void decode_entry(tc_ctx *ctx, const tc_block *blk, u8 *text, bool on_dev) {
    if (!blk || blk->n > TC_MAX_N || blk->sigma > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (blk->n == 0) return;
    if (!text || !blk->run_count || !blk->run_value || blk->nruns == 0)
        TC_FAIL(ctx, TC_ERR_ARG, "bad block");
    if (on_dev) return decode_device(ctx, blk, text);
    CallScope sc(ctx);
    u8 *d_text = sc.dev<u8>(blk->n + 16);
    u32 *d_count = sc.dev<u32>(blk->nruns);
    u16 *d_value = sc.dev<u16>(blk->nruns);
    tc_h2d(ctx, d_count, blk->run_count, blk->nruns * sizeof(u32));
    tc_h2d(ctx, d_value, blk->run_value, blk->nruns * sizeof(u16));
    tc_block dev = *blk;
    dev.run_count = d_count;
    dev.run_value = d_value;
    decode_device(ctx, &dev, d_text);
    tc_d2h(ctx, text, d_text, blk->n);
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
}

// ---- containers
static void encode_container_dev_entry(tc_ctx *ctx, const u8 *d_text, u64 n, u8 *d_out, u64 *bytes) {
    if (!bytes || n > TC_MAX_N || (n && !d_text)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    encode_container_device(ctx, d_text, n, d_out, bytes);
}
// host buffers in and out: text -> container.  The copy back is the compact form (an ACGTN record:
// 0.42 bytes per input byte instead of 4.8 for the raw runs).
static void encode_container_entry(tc_ctx *ctx, const u8 *text, u64 n, u8 *out, u64 *bytes) {
    if (!bytes || n > TC_MAX_N || (n && !text) || !out) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *bytes;
    // text in (staged through the context's page-locked ring unless the caller's buffer is page-locked), the record
    // straight into its container on the device (the call tc_encode_container_dev makes: the RLE stage writes the wire
    // format), the container out.  The device-side container is sized by what the caller can take, not by the worst case.
    u8 *d_text = hp_dev(ctx, 0, n + 16);
    const u64 need_max = container_bound_any(n);
    u64 dbytes = cap < need_max ? cap : need_max;
    if (dbytes < TC_CONTAINER_HEADER) dbytes = TC_CONTAINER_HEADER;
    u8 *d_out = hp_dev(ctx, 1, dbytes + 16);
    hp_copy(ctx, d_text, text, n, true);
    u64 used = cap < TC_CONTAINER_HEADER ? 0 : dbytes;   // (0 forces the capacity report)
    try {
        encode_container_device(ctx, d_text, n, d_out, &used);
    } catch (const TcFail &) {
        *bytes = used;
        throw;
    }
    *bytes = used;
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hp_copy(ctx, out, d_out, used, false);
}
// host buffers: container -> text (text must hold the n bytes tc_container_info reports)
static void decode_container_entry(tc_ctx *ctx, const u8 *container, u64 bytes, u8 *text, u64 *n_out) {
    if (!container || !n_out) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (bytes < TC_CONTAINER_HEADER) TC_FAIL(ctx, TC_ERR_MALFORMED, "container shorter than its header");
    const ContainerHeader h0 = container_header_parse(ctx, container, bytes, HDR_BOUNDS);
    if (h0.n && !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u8 *d_in = hp_dev(ctx, 0, bytes + 16);
    u8 *d_text = hp_dev(ctx, 1, h0.n + 16);
    u32 *d_count = reinterpret_cast<u32 *>(hp_dev(ctx, 2, (h0.nruns + 1) * sizeof(u32)));
    u16 *d_value = reinterpret_cast<u16 *>(hp_dev(ctx, 3, (h0.nruns + 1) * sizeof(u16)));
    hp_copy(ctx, d_in, container, bytes, true);
    tc_block dev;
    memset(&dev, 0, sizeof dev);
    dev.nruns = h0.nruns; dev.run_count = d_count; dev.run_value = d_value;
    container_read_device(ctx, d_in, bytes, &dev);
    *n_out = dev.n;
    if (dev.n) {
        if (dev.nruns == 0) TC_FAIL(ctx, TC_ERR_MALFORMED, "container holds no runs");
        decode_device(ctx, &dev, d_text);
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hp_copy(ctx, text, d_text, dev.n, false);
    }
}

// ================================================== chunked stream of containers
// A text of any length as independent records of block_bytes each (every record is its own
// BWT -> MTF -> RLE block, as bzip2 does with its blocks), written as containers back to back.
// The device works on record k while one helper thread copies record k+1 in and another copies
// container k-1 out, each on its own stream.  Both directions are the same two-slot loop around a different device step;
// they stay two loops: written once, over callables for the input span, the step and the destination, it came out
// longer than the two together.

// one copy on a stream of its own, made and waited for by a helper thread
struct CopyJob {
    std::thread th;
    hipError_t err = hipSuccess;
    void start(int device, hipStream_t s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        err = hipSuccess;
        if (!bytes) return;
        th = std::thread([this, device, s, dst, src, bytes, kind] {
            hipError_t e = hipSetDevice(device);
            if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, kind, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            err = e;
        });
    }
    hipError_t join() {
        if (th.joinable()) th.join();
        return err;
    }
    ~CopyJob() { (void)join(); }
};

static u64 stream_blocks(u64 n, u64 block) { return n ? (n + block - 1) / block : 1; }

// tc_encode_stream
static void encode_stream_entry(tc_ctx *ctx, const u8 *text, u64 n, u64 block_bytes, u8 *out, u64 *bytes) {
    if (block_bytes == 0) block_bytes = TC_STREAM_BLOCK_DEFAULT;
    if (!bytes || !out || (n && !text) || block_bytes > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *bytes;
    *bytes = 0;
    const u64 nb = stream_blocks(n, block_bytes);
    const u64 bmax = n < block_bytes ? n : block_bytes;      // longest record
    const u64 runs_cap = bmax + 2;
    const u64 cont_cap = container_bound_any(bmax);
    CallScope sc(ctx);
    const hipStream_t s_in = sc.stream(), s_out = sc.stream();
    u8 *d_text[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    for (int i = 0; i < (nb > 1 ? 2 : 1); i++) {
        d_text[i] = sc.dev<u8>(bmax + 16);
        d_out[i] = sc.dev<u8>(cont_cap + 16);
    }
    u32 *d_count = sc.dev<u32>(runs_cap + 1);
    u16 *d_value = sc.dev<u16>(runs_cap + 1);
    CopyJob outj, in;   // (behind the scope: joined before it frees anything, `in` first)
    auto len_of = [&](u64 k) { return k + 1 < nb ? block_bytes : n - (nb - 1) * block_bytes; };
    in.start(ctx->device, s_in, d_text[0], text, len_of(0), hipMemcpyHostToDevice);
    u64 off = 0;          // bytes of `out` written or being written
    for (u64 k = 0; k < nb; k++) {
        const int sl = (int)(k & 1);
        const u64 nk = len_of(k);
        TC_HIP(ctx, in.join());
        if (k + 1 < nb)
            in.start(ctx->device, s_in, d_text[sl ^ 1], text + (k + 1) * block_bytes, len_of(k + 1),
                     hipMemcpyHostToDevice);
        tc_block dev;
        memset(&dev, 0, sizeof dev);
        dev.nruns = runs_cap; dev.run_count = d_count; dev.run_value = d_value;
        if (nk) encode_device(ctx, d_text[sl], nk, &dev, runs_cap);
        else dev.nruns = 0;
        // d_out[sl] was last read by the copy of container k-2, joined before container k-1 started
        u64 used = cont_cap;
        container_write_device(ctx, &dev, d_out[sl], &used);
        TC_HIP(ctx, outj.join());
        if (off + used > cap) {
            *bytes = tc_stream_bound(n, block_bytes);
            TC_FAIL(ctx, TC_ERR_CAPACITY, "stream needs more than %llu bytes (bound %llu)",
                    (unsigned long long)cap, (unsigned long long)*bytes);
        }
        outj.start(ctx->device, s_out, out + off, d_out[sl], used, hipMemcpyDeviceToHost);
        off += used;
    }
    TC_HIP(ctx, outj.join());
    *bytes = off;
}

// tc_decode_stream
static void decode_stream_entry(tc_ctx *ctx, const u8 *stream, u64 bytes, u8 *text, u64 *n_out) {
    if (!n_out) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *n_out;
    *n_out = 0;
    const StreamIndex ix = stream_index(ctx, stream, bytes);
    if (ix.n_total > cap) {
        *n_out = ix.n_total;
        TC_FAIL(ctx, TC_ERR_CAPACITY, "text needs %llu bytes", (unsigned long long)ix.n_total);
    }
    if (ix.n_total && !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    const u64 nb = ix.off.size();
    CallScope sc(ctx);
    const hipStream_t s_in = sc.stream(), s_out = sc.stream();
    u8 *d_in[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr};
    for (int i = 0; i < (nb > 1 ? 2 : 1); i++) {
        d_in[i] = sc.dev<u8>(ix.len_max + 16);
        d_text[i] = sc.dev<u8>(ix.n_max + 16);
    }
    u32 *d_count = sc.dev<u32>(ix.nruns_max + 1);
    u16 *d_value = sc.dev<u16>(ix.nruns_max + 1);
    CopyJob outj, in;
    in.start(ctx->device, s_in, d_in[0], stream + ix.off[0], ix.len[0], hipMemcpyHostToDevice);
    u64 toff = 0;
    for (u64 k = 0; k < nb; k++) {
        const int sl = (int)(k & 1);
        TC_HIP(ctx, in.join());
        if (k + 1 < nb)
            in.start(ctx->device, s_in, d_in[sl ^ 1], stream + ix.off[k + 1], ix.len[k + 1],
                     hipMemcpyHostToDevice);
        tc_block dev;
        memset(&dev, 0, sizeof dev);
        dev.nruns = ix.nruns_max; dev.run_count = d_count; dev.run_value = d_value;
        container_read_device(ctx, d_in[sl], ix.len[k], &dev);
        if (dev.n != ix.n[k]) TC_FAIL(ctx, TC_ERR_MALFORMED, "container header changed");
        // d_text[sl] was last read by the copy of record k-2, joined before record k-1 started
        if (dev.n) {
            if (dev.nruns == 0) TC_FAIL(ctx, TC_ERR_MALFORMED, "container holds no runs");
            decode_device(ctx, &dev, d_text[sl]);
            TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        TC_HIP(ctx, outj.join());
        outj.start(ctx->device, s_out, text + toff, d_text[sl], dev.n, hipMemcpyDeviceToHost);
        toff += dev.n;
    }
    TC_HIP(ctx, outj.join());
    *n_out = toff;
}
