// textcomp.hip -- libtextcomp.so: C ABI (include/textcomp.h) over the HIP kernels.
// Single translation unit for gfx950: hipcc --offload-arch=gfx950 -shared -fPIC.
#include <thread>
#include <vector>

#include "tc_common.hpp"
#include "tc_encode_host.hpp"
#include "tc_decode_host.hpp"
#include "tc_fm_host.hpp"
#include "tc_lcp_host.hpp"
#include "tc_pack.hpp"
#include "tc_huff.hpp"
#include "tc_container_host.hpp"
#include "tc_comm.hpp"
#include "textcomp_debug.h"

// ================================================================== context
// The workspace.  Long records want it as physical chunks created one by one and mapped into one reserved,
// chunk-aligned address range (HIP virtual memory management) rather than as one hipMalloc block: with the
// single block the partition levels of a 1 GiB record run in their slow mode three times out of four (memory-
// side back-pressure: TCC_EA0_{WR,RD}REQ_DRAM_CREDIT_STALL 3.5x / 6x higher, address translation alike;
// profiles/r03_mode_pmc.txt), with chunks of 2^24 .. 2^34 bytes 30 fresh contexts of 32 landed in the fast one
// (profiles/r03_ws_recipes.txt).  TC_WS_VMM = log2 of the chunk size (default 28; 0: always
// hipMalloc); workspaces under 32 GiB (TC_WS_VMM_MIN_LOG2) are plain hipMalloc blocks.
struct TcWs {
    char *p = nullptr;
    size_t cap = 0, mapped = 0, reserved = 0;
    std::vector<hipMemGenericAllocationHandle_t> chunks;   // (mapped / chunks.size() bytes each)
};
static TcWs ws_detach(tc_ctx *ctx) {
    TcWs w;
    w.p = ctx->ws; w.cap = ctx->ws_cap; w.mapped = ctx->ws_mapped; w.reserved = ctx->ws_reserved;
    w.chunks.swap(ctx->ws_chunks);
    ctx->ws = nullptr; ctx->ws_cap = 0; ctx->ws_mapped = 0; ctx->ws_reserved = 0;
    return w;
}
static void ws_attach(tc_ctx *ctx, TcWs &w) {
    ctx->ws = w.p; ctx->ws_cap = w.cap; ctx->ws_mapped = w.mapped; ctx->ws_reserved = w.reserved;
    ctx->ws_chunks.swap(w.chunks);
    w = TcWs();
}
static void ws_free(TcWs &w) {
    if (!w.p) return;
    if (!w.chunks.empty()) {
        // hipFree waits for the whole device before it gives memory back; hipMemUnmap / hipMemRelease do NOT -- and a
        // kernel of ANOTHER stream (the exchange's, a caller's) may still be running over these pages.  Round 3 saw a
        // GPU memory fault after several chunked workspaces had been created and released in one process; since
        // then (round 4) a chunked workspace is never released while its context lives (it GROWS by mapping more
        // chunks into its reserved range: ws_grow_vmm), and where one is released -- the context's end -- the device
        // is idle first.
        (void)hipDeviceSynchronize();
        // every mapping is undone on its own (hipMemUnmap takes exactly one mapped range), then its memory
        // released; the address range goes last
        const size_t chunk = w.mapped / w.chunks.size();
        for (size_t i = 0; i < w.chunks.size(); i++) {
            if (hipMemUnmap(w.p + i * chunk, chunk) != hipSuccess) (void)hipGetLastError();
            if (hipMemRelease(w.chunks[i]) != hipSuccess) (void)hipGetLastError();
        }
        if (hipMemAddressFree(w.p, w.reserved ? w.reserved : w.mapped) != hipSuccess) (void)hipGetLastError();
    } else {
        (void)hipFree(w.p);
    }
    w = TcWs();
}
// more chunks of the same size behind the mapped ones, inside the reserved range: the workspace grows where it is, the
// pages a running kernel may hold stay mapped
static bool ws_grow_vmm(tc_ctx *ctx, size_t want) {
    if (ctx->ws_chunks.empty() || want > ctx->ws_reserved) return false;
    const size_t chunk = ctx->ws_mapped / ctx->ws_chunks.size();
    const size_t total = (want + chunk - 1) / chunk * chunk;
    if (total > ctx->ws_reserved) return false;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = ctx->device;
    const size_t from = ctx->ws_mapped;
    size_t done = from;
    const size_t n0 = ctx->ws_chunks.size();
    bool ok = true;
    for (; done < total; done += chunk) {
        hipMemGenericAllocationHandle_t h;
        if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) { ok = false; break; }
        if (hipMemMap(ctx->ws + done, chunk, 0, h, 0) != hipSuccess) { (void)hipMemRelease(h); ok = false; break; }
        ctx->ws_chunks.push_back(h);
    }
    if (ok && done > from) {
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        ok = hipMemSetAccess(ctx->ws + from, done - from, &acc, 1) == hipSuccess;
    }
    if (!ok) {   // (the new chunks only: nothing ever ran on them)
        (void)hipGetLastError();
        for (size_t i = n0; i < ctx->ws_chunks.size(); i++) {
            (void)hipMemUnmap(ctx->ws + i * chunk, chunk);
            (void)hipMemRelease(ctx->ws_chunks[i]);
        }
        ctx->ws_chunks.resize(n0);
        (void)hipGetLastError();
        return false;
    }
    ctx->ws_mapped = total;
    ctx->ws_cap = total;
    return true;
}
static bool ws_alloc_vmm(tc_ctx *ctx, size_t want, int chunk_log2, TcWs &w, bool growable = true) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = ctx->device;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) {
        (void)hipGetLastError();
        return false;
    }
    size_t chunk = (size_t)1 << chunk_log2;
    chunk = (chunk + gran - 1) / gran * gran;
    const size_t total = (want + chunk - 1) / chunk * chunk;
    // the address range: room for the workspace of the longest record (TC_WS_VMM_RESERVE_LOG2, default 2^38 bytes =
    // 256 GiB of addresses, not of memory), so that a context that meets a longer record later grows in place
    size_t reserve = growable ? (size_t)1 << env_int("TC_WS_VMM_RESERVE_LOG2", 38) : total;
    reserve = reserve / chunk * chunk;
    if (reserve < total) reserve = total;
    void *va = nullptr;
    if (hipMemAddressReserve(&va, reserve, chunk, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        reserve = total;
        if (hipMemAddressReserve(&va, reserve, chunk, nullptr, 0) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    }
    size_t done = 0;
    bool ok = true;
    for (; done < total; done += chunk) {
        hipMemGenericAllocationHandle_t h;
        if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) { ok = false; break; }
        if (hipMemMap((char *)va + done, chunk, 0, h, 0) != hipSuccess) { (void)hipMemRelease(h); ok = false; break; }
        w.chunks.push_back(h);
    }
    if (ok) {
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        ok = hipMemSetAccess(va, total, &acc, 1) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        for (size_t i = 0; i < w.chunks.size(); i++) {
            (void)hipMemUnmap((char *)va + i * chunk, chunk);
            (void)hipMemRelease(w.chunks[i]);
        }
        w.chunks.clear();
        (void)hipMemAddressFree(va, reserve);
        (void)hipGetLastError();
        return false;
    }
    w.p = (char *)va; w.cap = total; w.mapped = total; w.reserved = reserve;
    return true;
}
// a workspace of `want` bytes (exactly `want` when exact: a second placement of an existing size)
static bool ws_alloc(tc_ctx *ctx, size_t want, TcWs &w) {
    const int vmm = env_int("TC_WS_VMM", 28);
    // (from TC_WS_VMM_MIN_LOG2 = 2^35 bytes on: the workspace of a record of about 2^29 bytes -- where the two modes
    // of the partition levels are worth avoiding; smaller workspaces are plain blocks)
    const size_t vmm_min = (size_t)1 << env_int("TC_WS_VMM_MIN_LOG2", 35);
    if (vmm >= 21 && vmm <= 36 && want >= vmm_min && ws_alloc_vmm(ctx, want, vmm, w)) return true;
    if (hipMalloc((void **)&w.p, want) != hipSuccess) {
        (void)hipGetLastError();
        w.p = nullptr;
        return false;
    }
    w.cap = want;
    return true;
}
void *tc_chunked_alloc(tc_ctx *ctx, size_t bytes, int chunk_log2, void **handle) {
    TcWs *w = new TcWs();
    if (!ws_alloc_vmm(ctx, bytes, chunk_log2, *w, /*growable=*/false)) {   // (no spare address range: this block never grows)
        delete w;
        return nullptr;
    }
    *handle = w;
    return w->p;
}
void tc_chunked_free(void *handle) {
    TcWs *w = static_cast<TcWs *>(handle);
    if (!w) return;
    ws_free(*w);
    delete w;
}
static void tc_ws_release(tc_ctx *ctx) {
    TcWs w = ws_detach(ctx);
    ws_free(w);
}

void tc_ws_reserve(tc_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->ws_cap) return;
    // a chunked workspace grows where it is (more chunks behind the mapped ones): no release, no new placement
    if (ctx->ws && !ctx->ws_chunks.empty() && ws_grow_vmm(ctx, bytes + (bytes >> 4) + (1u << 20))) {
        ctx->stats_ws_grown++;
        return;
    }
    if (ctx->ws) {
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        tc_ws_release(ctx);
    }
    TcWs w;
    if (!ws_alloc(ctx, bytes + (bytes >> 4) + (1u << 20), w) && !ws_alloc(ctx, bytes, w))
        TC_FAIL(ctx, TC_ERR_OOM, "workspace of %zu bytes: out of device memory", bytes);
    ws_attach(ctx, w);
}

u32 tc_persistent_grid(tc_ctx *ctx, int blocks_per_cu) {
    int pct = env_int("TC_GRID_SCALE_PCT", 100);
    u64 g = (u64)ctx->num_cus * (u64)blocks_per_cu * (u64)pct / 100;
    return g < 1 ? 1u : (u32)g;
}

void tc_sync_check(tc_ctx *ctx) {
    u32 err = 0;
    TC_HIP(ctx, hipMemcpyAsync(&ctx->h_scalars[63], ctx->d_err, sizeof(u32), hipMemcpyDeviceToHost,
                               ctx->stream));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    err = (u32)ctx->h_scalars[63];
    if (err) {
        (void)hipMemsetAsync(ctx->d_err, 0, sizeof(u32), ctx->stream);
        if (err & 0xff00u) TC_FAIL(ctx, TC_ERR_MALFORMED, "malformed input (device flag 0x%x)", err);
        TC_FAIL(ctx, TC_ERR_INTERNAL, "device-side failure flag 0x%x", err);
    }
}

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
    tc_ws_reserve(ctx, dry.off);
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
static void mtf_host(tc_ctx *ctx, const void *src, size_t src_bytes, bool is_sym, u64 N,
                     i64 primary, u16 *idx, i16 *final_list, u32 *sigma) {
    u8 *d_src = nullptr;
    u16 *d_idx = nullptr;
    auto plan = [&](Arena &A, bool dry) {
        d_src = A.get<u8>(src_bytes + 16);
        d_idx = A.get<u16>(N);
        if (!dry) tc_h2d(ctx, d_src, src, src_bytes);
        Acc acc = make_acc<Acc>(d_src, primary);
        (void)is_sym;
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


__device__ __forceinline__ u64 gen_mix(u64 seed, u64 i) {   // splitmix64 of (seed, position): SURVEY.md 8(d)
    u64 z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ u32 gen_scaled(u64 z, u32 m) { return (u32)(((z >> 32) * (u64)m) >> 32); }   // uniform over 0 .. m - 1
__device__ __forceinline__ u8 gen_acgt(u32 k) { return (u8)(0x54474341u >> (8 * (k & 3u))); }

// Every byte is a function of (kind, seed, position) alone (integer arithmetic; no state carried along the text):
//   0 iid ACGTN, 1 printable ASCII;  the classes away from iid text the bench reports (round 4):
//   2 genome-like: iid ACGT; per 3000-byte cell one copy of a 300-bp family at a hashed offset, 15 % of its bases redrawn;
//     per 20 000-byte cell a poly-A tract of 15 .. 59; per 100 000-byte cell 100 bytes of (CA)n
//   4 runs: a new run starts at a position with probability 1/10, the run's letter is drawn at its start
//   5 periodic: a 4096-byte iid ACGT block repeated
//   6 an assembly with gaps: iid ACGT with runs of 'N' (a function of the position AND the length n)
// (3, Zipf words, needs the word boundaries: generate_words_kernel below)
__global__ __launch_bounds__(256) void generate_kernel(int kind, u64 seed, u64 n, u8 *out) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 z = gen_mix(seed, i);
        const u32 hi = (u32)(z >> 32);
        u8 b;
        if (kind == 0) {
            u32 k = (u32)(((u64)hi * 5) >> 32);
            b = (u8)(0x4E54474341ull >> (8 * k));  // "ACGTN"
        } else if (kind == 1) {
            b = (u8)(0x20 + (u32)(((u64)hi * 95) >> 32));
        } else if (kind == 2) {
            b = gen_acgt(gen_scaled(z, 4));
            const u64 c3 = i / 3000, o3 = i % 3000;
            const u32 f0 = gen_scaled(gen_mix(seed + 2, c3), 2700);
            if (o3 >= f0 && o3 < f0 + 300) {
                const u64 x = gen_mix(seed + 3, i);
                b = gen_scaled(x, 100) < 15 ? gen_acgt((u32)(x >> 8)) : gen_acgt(gen_scaled(gen_mix(seed + 1, o3 - f0), 4));
            }
            const u64 c2 = i / 20000, o2 = i % 20000;
            const u32 a0 = gen_scaled(gen_mix(seed + 4, c2), 19900), al = 15 + gen_scaled(gen_mix(seed + 5, c2), 45);
            if (o2 >= a0 && o2 < a0 + al) b = 65;
            const u64 c1 = i / 100000, o1 = i % 100000;
            const u32 m0 = gen_scaled(gen_mix(seed + 6, c1), 99800);
            if (o1 >= m0 && o1 < m0 + 100) b = ((o1 - m0) & 1) ? 65 : 67;
        } else if (kind == 4) {
            u64 j = i;
            for (int back = 0; back < 512 && j > 0 && gen_scaled(gen_mix(seed, j), 10) != 0; back++) j--;
            b = gen_acgt((u32)(gen_mix(seed + 1, j) >> 40));
        } else if (kind == 6) {
            // an assembly with gaps: iid ACGT, one run of n / 64 'N's from n / 3 on, sixteen of n / 4096 at the odd multiples of n / 40
            b = gen_acgt(gen_scaled(z, 4));
            const u64 g0 = n / 3, cell = n / 40;
            if (i >= g0 && i < g0 + n / 64) b = 78;
            else if (cell) {
                const u64 c = i / cell;
                if ((c & 1) && c < 32 && i - c * cell < n / 4096) b = 78;
            }
        } else {
            b = gen_acgt(gen_scaled(gen_mix(seed, i & 4095), 4));
        }
        out[i] = b;
    }
}
// kind 3, natural-language-like: words drawn Zipf(1) from a 20 000-word vocabulary (2 .. 9 lower-case letters, a space behind
// each).  One thread writes one 4096-byte cell, word after word from the cell's own counter stream (the last word of a cell
// is cut at the cell's end), so a byte is still a function of (seed, position) alone.  cw: cumulative integer weights.
#define GEN_VOCAB 20000
__global__ __launch_bounds__(256) void generate_vocab_kernel(u64 seed, u64 *cw_scratch) {
    // weights 2^40 / (k + 1); the running sum is made by generate_cw_kernel (one thread: 20 000 additions)
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k < GEN_VOCAB) cw_scratch[k] = (1ull << 40) / (u64)(k + 1);
    (void)seed;
}
__global__ void generate_cw_kernel(u64 *cw) {
    u64 run = 0;
    for (u32 k = 0; k < GEN_VOCAB; k++) { run += cw[k]; cw[k] = run; }
}
__global__ __launch_bounds__(64) void generate_words_kernel(u64 seed, u64 n, const u64 *__restrict__ cw, u8 *out) {
    const u64 cell = (u64)blockIdx.x * 64 + threadIdx.x;
    const u64 base = cell * 4096;
    if (base >= n) return;
    const u64 end = base + 4096 < n ? base + 4096 : n;
    const u64 total = cw[GEN_VOCAB - 1];
    u64 p = base;
    for (u64 w = 0; p < end; w++) {
        const u64 u = (gen_mix(seed + 3, cell * 4096 + w) >> 20) % total;
        u32 lo = 0, hi = GEN_VOCAB - 1;   // first k with cw[k] > u
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (cw[mid] > u) hi = mid; else lo = mid + 1;
        }
        const u32 len = 2 + (u32)(gen_mix(seed + 1, lo) % 8);
        for (u32 t = 0; t < len && p < end; t++, p++) out[p] = (u8)(97 + gen_mix(seed + 2, (u64)lo * 16 + t) % 26);
        if (p < end) out[p++] = 32;
    }
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

// ------------------------------------------------------------ calibration kernels
template <class T>
__global__ __launch_bounds__(256) void dbg_stream_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                         u64 count, int mode, u32 *sink) {
    u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 stride = (u64)gridDim.x * 256;
    if (mode == 0) {
        for (; i < count; i += stride) out[i] = in[i];
    } else if (mode == 1) {
        u32 acc = 0;
        for (; i < count; i += stride) {
            T v = in[i];
            const unsigned char *p = reinterpret_cast<const unsigned char *>(&v);
            acc += p[0];
        }
        if (acc == 0x12345678u) *sink = acc;
    } else {
        T v;
        memset(&v, 7, sizeof(T));
        for (; i < count; i += stride) out[i] = v;
    }
}
template <class T>
static double dbg_stream_run(tc_ctx *ctx, char *a, char *b, u64 bytes, int mode, int iters) {
    const u64 count = bytes / sizeof(T);
    u32 grid = tc_cdiv(count, 256 * 8);
    if (grid > 256u * 16u * 4u) grid = 256u * 16u * 4u;
    hipStream_t s = ctx->stream;
    dbg_stream_kernel<T><<<grid, 256, 0, s>>>((const T *)a, (T *)b, count, mode, ctx->d_err + 8);
    TC_LAUNCH_CHECK(ctx);
    TC_HIP(ctx, hipEventRecord(ctx->ev[6], s));
    for (int i = 0; i < iters; i++)
        dbg_stream_kernel<T><<<grid, 256, 0, s>>>((const T *)a, (T *)b, count, mode, ctx->d_err + 8);
    TC_HIP(ctx, hipEventRecord(ctx->ev[7], s));
    TC_HIP(ctx, hipStreamSynchronize(s));
    float ms = 0;
    TC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]));
    double moved = (double)count * sizeof(T) * (mode == 0 ? 2.0 : 1.0) * iters;
    return moved / (ms * 1e-3) / 1e9;
}

// memory pattern of one radix pass without any of its work: a tile of 4096 (key, value) pairs is
// read coalesced and written as `bins` segments, segment d of tile t behind segment d of tile t-1
// (what the scatter of a pass over uniformly distributed digits looks like to the memory system)
__global__ __launch_bounds__(256) void dbg_scatter_kernel(const u64 *__restrict__ kin, const u32 *__restrict__ vin,
                                                          u64 *__restrict__ kout, u32 *__restrict__ vout,
                                                          u32 ntiles, u32 bins, u32 xrun) {
    u32 t = blockIdx.x;
    const u32 xr = xrun & 255u;
    if (xr) {  // XCD-aware order: blocks with equal blockIdx % 8 take tiles in runs of `xr`
        const u32 x = blockIdx.x & 7u, a = blockIdx.x >> 3, G = ntiles / (8 * xr);
        if (a < G * xr) t = (a / xr) * (8 * xr) + x * xr + (a % xr);
    }
    const u64 base = (u64)t * 4096;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const u32 e = threadIdx.x + k * 256;
        const u64 key = kin[base + e];
        const u32 val = vin[base + e];
        const u32 d = (u32)(((u64)e * bins) >> 12);
        u32 lo = (d * 4096u + bins - 1) / bins;            // first element of segment d
        u32 hi = ((d + 1) * 4096u + bins - 1) / bins;
        const u64 sbeg = (u64)lo * ntiles + (u64)t * (hi - lo), send = sbeg + (hi - lo);
        const u64 o = sbeg + (e - lo);
        const int nt = (int)(xrun >> 8);   // experiment: 1 = all stores non-temporal, 2 = only those into lines this tile fills alone
        bool knt = nt == 1, vnt = nt == 1;
        if (nt == 2) {
            const u64 kl0 = o & ~15ull, vl0 = o & ~31ull;
            knt = kl0 >= sbeg && kl0 + 16 <= send;
            vnt = vl0 >= sbeg && vl0 + 32 <= send;
        }
        if (knt) __builtin_nontemporal_store(key, kout + o); else kout[o] = key;
        if (vnt) __builtin_nontemporal_store(val, vout + o); else vout[o] = val;
    }
}

__global__ __launch_bounds__(256) void dbg_random_keys_kernel(u64 *keys, u64 n, u64 seed, int key_bits) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        u64 z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        keys[i] = (z << (64 - key_bits)) | (i & 0xff);
    }
}
// sorted by the top bits, and stable: equal keys keep increasing values
__global__ __launch_bounds__(256) void dbg_check_sorted_kernel(const u64 *keys, const u32 *vals, u64 n,
                                                               int key_bits, u32 *bad) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i + 1 < n; i += (u64)gridDim.x * 256) {
        u64 a = keys[i] >> (64 - key_bits), b = keys[i + 1] >> (64 - key_bits);
        if (a > b || (a == b && vals[i] >= vals[i + 1])) atomicAdd(bad, 1u);
    }
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

static void hp_release(tc_ctx *ctx);
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
    if (!out || !d_text || n == 0 || n > TC_MAX_N || tries < 1 || !out->run_count || !out->run_value)
        TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (tries > 8) tries = 8;
    const u64 cap = out->nruns;
    std::vector<double> t;
    std::vector<char *> spacers;
    auto timed = [&]() {
        double best = 1e30;
        for (int rep = 0; rep < 3; rep++) {   // (the first encode on a new block is not counted: first touch)
            TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const auto t0 = std::chrono::steady_clock::now();
            tc_block b = *out;
            b.nruns = cap;
            encode_device(ctx, d_text, n, &b, cap);
            TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const double m = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rep > 0 && m < best) best = m;
            if (rep == 2) *out = b;
        }
        return best;
    };
    int best = 0;
    TcWs best_ws;                       // the best placement so far while a candidate is attached to the context
    auto release = [&]() {
        for (char *sp : spacers) (void)hipFree(sp);
        spacers.clear();
    };
    try {
        t.push_back(timed());          // placement 0: the workspace the context has (sized by this very encode)
        const size_t cap0 = ctx->ws_cap;
        // A workspace of mapped chunks (the default for long records) is not placed again: it lands in the fast
        // mode by itself (profiles/r03_ws_recipes.txt), and one bench run whose search created and released
        // several 80 GB chunked workspaces in a row ended in a GPU memory fault that no run with a single one
        // ever showed -- cause not established (hipMemUnmap over all mappings at once returns success, so it was
        // not the release as first suspected; scripts/dbg/vmm_unmap_probe.cpp), so the search stays with
        // hipMalloc blocks (TC_WS_VMM=0), where round 2 ran it hundreds of times.
        if (!ctx->ws_chunks.empty()) tries = 1;
        for (int k = 1; k < tries; k++) {
            double worst = 0;
            for (double v : t) worst = v > worst ? v : worst;
            // two modes ~7 % apart: once both have been seen the faster one is known
            if (t[best] < 0.96 * worst && env_int("TC_PLACE_ALL", 0) == 0) break;   // (TC_PLACE_ALL=1: experiments)
            size_t free_b = 0, total_b = 0;
            TC_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
            if (free_b < cap0 + ((size_t)8 << 30)) break;     // no room for a second workspace
            TcWs cand;
            if (!ws_alloc(ctx, cap0, cand)) break;
            best_ws = ws_detach(ctx);  // (the best one so far stays allocated: the candidate lands elsewhere)
            ws_attach(ctx, cand);
            t.push_back(timed());
            if (ctx->ws_cap < cap0 || ctx->ws_cap > cap0 + ((size_t)1 << 30)) {   // re-reserved under the candidate: keep it
                ws_free(best_ws);
                best = k;
                break;
            }
            if (t[k] < t[best]) {
                best = k;
                ws_free(best_ws);
            } else {
                TcWs loser = ws_detach(ctx);
                ws_attach(ctx, best_ws);
                const bool plain = loser.chunks.empty();
                ws_free(loser);
                // a spacer in the hole a rejected block leaves: the next candidate does not fit there and goes somewhere new
                char *sp = nullptr;
                if (plain && hipMalloc((void **)&sp, (size_t)1 << 30) == hipSuccess) spacers.push_back(sp);
                else (void)hipGetLastError();
            }
        }
    } catch (const TcFail &) {
        if (best_ws.p) {               // reinstate the best workspace, with its capacity, whatever the candidate became
            tc_ws_release(ctx);
            ws_attach(ctx, best_ws);
        }
        release();
        throw;
    }
    release();
    if (ms)
        for (int k = 0; k < tries; k++) ms[k] = k < (int)t.size() ? t[k] : 0.0;
    if (chosen) *chosen = best;
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
    if (n > TC_MAX_N || !primary) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) { *primary = 0; return TC_OK; }  // BWT.hs:58
    if (!d_text || !d_L) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    ctx->stats = tc_stats{};
    ctx->stats.n = n; ctx->stats.N = n + 1;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool dry) { sa_build(ctx, A, d_text, n, nullptr, d_L, primary, nullptr, dry); });
    tc_sync_check(ctx);
    TC_API_END(ctx)
}

int tc_bwt_encode(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *L, uint64_t *primary) {
    TC_API_BEGIN(ctx)
    if (n > TC_MAX_N || !primary) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) { *primary = 0; return TC_OK; }
    if (!text || !L) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    bwt_host(ctx, text, n, L, nullptr, primary);
    TC_API_END(ctx)
}

int tc_suffix_array(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t *sa) {
    TC_API_BEGIN(ctx)
    if (n > TC_MAX_N || !sa) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (n == 0) { sa[0] = 0; return TC_OK; }
    if (!text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    u64 primary;
    bwt_host(ctx, text, n, nullptr, sa, &primary);
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

// ================================================================= Data.MTF
int tc_mtf_encode(tc_ctx *ctx, const uint8_t *L, uint64_t N, int64_t primary, uint16_t *idx,
                  int16_t *final_list, uint32_t *sigma) {
    TC_API_BEGIN(ctx)
    if (!sigma || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *sigma = 0; return TC_OK; }  // MTF/Internal.hs:129-132
    if (!L || !idx || !final_list || primary >= (i64)N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    mtf_host<BwtAcc>(ctx, L, N, false, N, primary < 0 ? -1 : primary, idx, final_list, sigma);
    TC_API_END(ctx)
}

int tc_mtf_encode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint16_t *idx,
                      int16_t *final_list, uint32_t *sigma) {
    TC_API_BEGIN(ctx)
    if (!sigma || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *sigma = 0; return TC_OK; }
    if (!sym || !idx || !final_list) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    mtf_host<SymAcc>(ctx, sym, N * sizeof(i16), true, N, -1, idx, final_list, sigma);
    TC_API_END(ctx)
}

// ================================================================= Data.RLE
int tc_rle_encode(tc_ctx *ctx, const uint8_t *L, uint64_t N, int64_t primary, uint32_t *counts,
                  int16_t *syms, uint64_t *nruns) {
    TC_API_BEGIN(ctx)
    if (!nruns || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *nruns = 0; return TC_OK; }  // RLE.hs:119
    if (!L || !counts || !syms || primary >= (i64)N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    rle_host<BwtAcc, i16>(ctx, L, N, N, primary < 0 ? -1 : primary, counts, syms, nruns);
    TC_API_END(ctx)
}

int tc_rle_encode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint32_t *counts,
                      int16_t *syms, uint64_t *nruns) {
    TC_API_BEGIN(ctx)
    if (!nruns || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *nruns = 0; return TC_OK; }  // RLE.hs:157
    if (!sym || !counts || !syms) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    rle_host<SymAcc, i16>(ctx, sym, N * sizeof(i16), N, -1, counts, syms, nruns);
    TC_API_END(ctx)
}

int tc_rle_encode_u16(tc_ctx *ctx, const uint16_t *vals, uint64_t N, uint32_t *counts,
                      uint16_t *run_vals, uint64_t *nruns) {
    TC_API_BEGIN(ctx)
    if (!nruns || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) { *nruns = 0; return TC_OK; }
    if (!vals || !counts || !run_vals) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    rle_host<U16Acc, u16>(ctx, vals, N * sizeof(u16), N, -1, counts, run_vals, nruns);
    TC_API_END(ctx)
}

// ============================================================ fused pipeline
int tc_encode_dev(tc_ctx *ctx, const uint8_t *d_text, uint64_t n, tc_block *out) {
    TC_API_BEGIN(ctx)
    if (!out || n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = out->nruns;
    out->n = n; out->primary = 0; out->sigma = 0; out->nruns = 0;
    if (n == 0) {              // empty in, empty out (BWT.hs:58, MTF.hs:157, RLE.hs:119)
        ctx->stats = tc_stats{};   // (the stats describe this call alone: encode_device resets them otherwise)
        return TC_OK;
    }
    if (!d_text || !out->run_count || !out->run_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    encode_device(ctx, d_text, n, out, cap);
    TC_API_END(ctx)
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

int tc_encode(tc_ctx *ctx, const uint8_t *text, uint64_t n, tc_block *out) {
    TC_API_BEGIN(ctx)
    if (!out || n > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = out->nruns;
    u32 *h_count = out->run_count;
    u16 *h_value = out->run_value;
    out->n = n; out->primary = 0; out->sigma = 0; out->nruns = 0;
    if (n == 0) {
        ctx->stats = tc_stats{};   // (the stats describe this call alone: encode_device resets them otherwise)
        return TC_OK;
    }
    if (!text || !h_count || !h_value) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
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
    TC_API_END(ctx)
}

// ============================================================ synthetic input
int tc_generate_dev(tc_ctx *ctx, int kind, uint64_t seed, uint64_t n, uint8_t *d_out) {
    TC_API_BEGIN(ctx)
    if (kind < 0 || kind > 6) TC_FAIL(ctx, TC_ERR_ARG, "bad kind");
    if (n == 0) return TC_OK;
    if (!d_out) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    if (kind == 3) {
        u64 *cw = nullptr;
        TC_HIP(ctx, hipMalloc((void **)&cw, GEN_VOCAB * sizeof(u64)));
        generate_vocab_kernel<<<tc_cdiv(GEN_VOCAB, 256), 256, 0, ctx->stream>>>(seed, cw);
        generate_cw_kernel<<<1, 1, 0, ctx->stream>>>(cw);
        generate_words_kernel<<<tc_cdiv(tc_cdiv(n, 4096), 64), 64, 0, ctx->stream>>>(seed, n, cw, d_out);
        const hipError_t e = hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(cw);
        TC_HIP(ctx, e);
    } else {
        u32 grid = tc_cdiv(n, 256 * 16);
        if (grid > 4096) grid = 4096;
        generate_kernel<<<grid, 256, 0, ctx->stream>>>(kind, seed, n, d_out);
        TC_LAUNCH_CHECK(ctx);
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    TC_API_END(ctx)
}


// ===================================================================== decode
int tc_bwt_decode(tc_ctx *ctx, const uint8_t *L, uint64_t N, uint64_t primary, uint8_t *text) {
    TC_API_BEGIN(ctx)
    if (N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0) return TC_OK;
    if (!L || !text || primary >= N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    u64 n_out = 0;
    ibwt_host<BwtAcc>(ctx, L, N, N, (i64)primary, text, &n_out);
    if (n_out != N - 1) TC_FAIL(ctx, TC_ERR_ARG, "not the BWT of any text (cycle of %llu rows)",
                                (unsigned long long)(n_out + 1));
    TC_API_END(ctx)
}

int tc_bwt_decode_sym(tc_ctx *ctx, const int16_t *sym, uint64_t N, uint8_t *text, uint64_t *n_out) {
    TC_API_BEGIN(ctx)
    if (!n_out || N > TC_MAX_N + 1) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    *n_out = 0;
    if (N == 0) return TC_OK;  // BWT/Internal.hs:164-167
    if (!sym || !text) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    ibwt_host<SymAcc>(ctx, sym, N * sizeof(i16), N, -1, text, n_out);
    TC_API_END(ctx)
}

int tc_mtf_decode(tc_ctx *ctx, const uint16_t *idx, uint64_t N, const int16_t *list,
                  uint32_t nlist, int16_t *sym) {
    TC_API_BEGIN(ctx)
    if (N > TC_MAX_N + 1 || nlist > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (N == 0 || nlist == 0) return TC_OK;  // MTF/Internal.hs:202-209
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
    TC_API_END(ctx)
}

int tc_rle_decode(tc_ctx *ctx, const uint32_t *counts, const int16_t *syms, uint64_t nruns,
                  int16_t *sym_out, uint64_t *N) {
    TC_API_BEGIN(ctx)
    if (!N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (nruns == 0) { *N = 0; return TC_OK; }  // RLE/Internal.hs:156-159
    if (!counts || !syms || (!sym_out && *N)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    rle_decode_host<i16>(ctx, counts, syms, nruns, true, sym_out, N);
    TC_API_END(ctx)
}

int tc_rle_decode_u16(tc_ctx *ctx, const uint32_t *counts, const uint16_t *run_vals,
                      uint64_t nruns, uint16_t *vals_out, uint64_t *N) {
    TC_API_BEGIN(ctx)
    if (!N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (nruns == 0) { *N = 0; return TC_OK; }
    if (!counts || !run_vals || (!vals_out && *N)) TC_FAIL(ctx, TC_ERR_ARG, "null buffer");
    rle_decode_host<u16>(ctx, counts, run_vals, nruns, false, vals_out, N);
    TC_API_END(ctx)
}

int tc_decode_dev(tc_ctx *ctx, const tc_block *blk, uint8_t *d_text) {
    TC_API_BEGIN(ctx)
    if (!blk || blk->n > TC_MAX_N || blk->sigma > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (blk->n == 0) return TC_OK;
    if (!d_text || !blk->run_count || !blk->run_value || blk->nruns == 0)
        TC_FAIL(ctx, TC_ERR_ARG, "bad block");
    decode_device(ctx, blk, d_text);
    TC_API_END(ctx)
}

int tc_decode(tc_ctx *ctx, const tc_block *blk, uint8_t *text) {
    TC_API_BEGIN(ctx)
    if (!blk || blk->n > TC_MAX_N || blk->sigma > TC_MAX_SIGMA) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (blk->n == 0) return TC_OK;
    if (!text || !blk->run_count || !blk->run_value || blk->nruns == 0)
        TC_FAIL(ctx, TC_ERR_ARG, "bad block");
    u8 *d_text = nullptr;
    u32 *d_count = nullptr;
    u16 *d_value = nullptr;
    int rc = TC_OK;
    try {
        TC_HIP(ctx, hipMalloc((void **)&d_text, blk->n + 16));
        TC_HIP(ctx, hipMalloc((void **)&d_count, blk->nruns * sizeof(u32)));
        TC_HIP(ctx, hipMalloc((void **)&d_value, blk->nruns * sizeof(u16)));
        tc_h2d(ctx, d_count, blk->run_count, blk->nruns * sizeof(u32));
        tc_h2d(ctx, d_value, blk->run_value, blk->nruns * sizeof(u16));
        tc_block dev = *blk;
        dev.run_count = d_count;
        dev.run_value = d_value;
        decode_device(ctx, &dev, d_text);
        tc_d2h(ctx, text, d_text, blk->n);
        TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } catch (const TcFail &f) {
        rc = f.code;
    }
    (void)hipStreamSynchronize(ctx->stream);
    if (d_text) (void)hipFree(d_text);
    if (d_count) (void)hipFree(d_count);
    if (d_value) (void)hipFree(d_value);
    if (rc != TC_OK) throw TcFail{rc};
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
    if (!bytes || n > TC_MAX_N || (n && !d_text)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    encode_container_device(ctx, d_text, n, d_out, bytes);
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

// host buffers in and out: text -> container.  The copy back is the compact form (an ACGTN record:
// 0.42 bytes per input byte instead of 4.8 for the raw runs).
int tc_encode_container(tc_ctx *ctx, const uint8_t *text, uint64_t n, uint8_t *out, uint64_t *bytes) {
    TC_API_BEGIN(ctx)
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
    TC_API_END(ctx)
}

// host buffers: container -> text (text must hold the n bytes tc_container_info reports)
int tc_decode_container(tc_ctx *ctx, const uint8_t *container, uint64_t bytes, uint8_t *text, uint64_t *n_out) {
    TC_API_BEGIN(ctx)
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
    TC_API_END(ctx)
}

// ================================================== chunked stream of containers
// A text of any length as independent records of block_bytes each (every record is its own
// BWT -> MTF -> RLE block, as bzip2 does with its blocks), written as containers back to back.
// The device works on record k while one helper thread copies record k+1 in and another copies
// container k-1 out, each on its own stream.
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
    if (block_bytes == 0) block_bytes = TC_STREAM_BLOCK_DEFAULT;
    if (!bytes || !out || (n && !text) || block_bytes > TC_MAX_N) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u64 cap = *bytes;
    *bytes = 0;
    const u64 nb = stream_blocks(n, block_bytes);
    const u64 bmax = n < block_bytes ? n : block_bytes;      // longest record
    const u64 runs_cap = bmax + 2;
    const u64 cont_cap = container_bound_any(bmax);
    u8 *d_text[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    u32 *d_count = nullptr;
    u16 *d_value = nullptr;
    hipStream_t s_in = nullptr, s_out = nullptr;
    int rc = TC_OK;
    {
        CopyJob in, outj;
        try {
            TC_HIP(ctx, hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
            TC_HIP(ctx, hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
            for (int i = 0; i < (nb > 1 ? 2 : 1); i++) {
                TC_HIP(ctx, hipMalloc((void **)&d_text[i], bmax + 16));
                TC_HIP(ctx, hipMalloc((void **)&d_out[i], cont_cap + 16));
            }
            TC_HIP(ctx, hipMalloc((void **)&d_count, (runs_cap + 1) * sizeof(u32)));
            TC_HIP(ctx, hipMalloc((void **)&d_value, (runs_cap + 1) * sizeof(u16)));
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
        } catch (const TcFail &f) {
            rc = f.code;
        }
        (void)in.join();
        (void)outj.join();
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 2; i++) {
        if (d_text[i]) (void)hipFree(d_text[i]);
        if (d_out[i]) (void)hipFree(d_out[i]);
    }
    if (d_count) (void)hipFree(d_count);
    if (d_value) (void)hipFree(d_value);
    if (s_in) (void)hipStreamDestroy(s_in);
    if (s_out) (void)hipStreamDestroy(s_out);
    if (rc != TC_OK) throw TcFail{rc};
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
    u8 *d_in[2] = {nullptr, nullptr}, *d_text[2] = {nullptr, nullptr};
    u32 *d_count = nullptr;
    u16 *d_value = nullptr;
    hipStream_t s_in = nullptr, s_out = nullptr;
    int rc = TC_OK;
    {
        CopyJob in, outj;
        try {
            TC_HIP(ctx, hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
            TC_HIP(ctx, hipStreamCreateWithFlags(&s_out, hipStreamNonBlocking));
            for (int i = 0; i < (nb > 1 ? 2 : 1); i++) {
                TC_HIP(ctx, hipMalloc((void **)&d_in[i], ix.len_max + 16));
                TC_HIP(ctx, hipMalloc((void **)&d_text[i], ix.n_max + 16));
            }
            TC_HIP(ctx, hipMalloc((void **)&d_count, (ix.nruns_max + 1) * sizeof(u32)));
            TC_HIP(ctx, hipMalloc((void **)&d_value, (ix.nruns_max + 1) * sizeof(u16)));
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
        } catch (const TcFail &f) {
            rc = f.code;
        }
        (void)in.join();
        (void)outj.join();
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 2; i++) {
        if (d_in[i]) (void)hipFree(d_in[i]);
        if (d_text[i]) (void)hipFree(d_text[i]);
    }
    if (d_count) (void)hipFree(d_count);
    if (d_value) (void)hipFree(d_value);
    if (s_in) (void)hipStreamDestroy(s_in);
    if (s_out) (void)hipStreamDestroy(s_out);
    if (rc != TC_OK) throw TcFail{rc};
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

int tc_fm_info(const tc_fm *fm, uint64_t *N, uint32_t *sigma, int16_t *c_sym, uint64_t *c_val,
               uint64_t *primary) {
    return fm_info(fm, N, sigma, c_sym, c_val, primary);
}


// ======================================================== multi-GPU exchange (RCCL, bound at run time)
int tc_comm_unique_id(tc_ctx *ctx, uint8_t *id) {
    TC_API_BEGIN(ctx)
    if (!id) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    std::string why;
    RcclApi *api = rccl_api(&why);
    if (!api) TC_FAIL(ctx, TC_ERR_NCCL, "%s", why.c_str());
    RcclId u;
    const int r = api->GetUniqueId(&u);
    if (r != 0) TC_FAIL(ctx, TC_ERR_NCCL, "ncclGetUniqueId -> %s", api->GetErrorString(r));
    memcpy(id, u.internal, TC_COMM_ID_BYTES);
    TC_API_END(ctx)
}

int tc_comm_create(tc_ctx *ctx, const uint8_t *id, int rank, int world, tc_comm **out) {
    TC_API_BEGIN(ctx)
    if (!id || !out || world < 1 || rank < 0 || rank >= world) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    *out = nullptr;
    std::string why;
    RcclApi *api = rccl_api(&why);
    if (!api) TC_FAIL(ctx, TC_ERR_NCCL, "%s", why.c_str());
    tc_comm *c = new tc_comm();
    c->ctx = ctx; c->api = api; c->rank = rank; c->world = world;
    try {
        // The exchange overlaps the next record's encode, and the partition levels of that encode want whole CUs
        // (one 1024-thread workgroup with 153 KB of LDS each, a static split of the work over the workgroups): an
        // RCCL workgroup resident on a CU for the ~10 ms of a transfer would hold one partition workgroup back and
        // with it the whole level.  So the two are kept apart by construction: the communicator's stream is
        // restricted to the last TC_COMM_CUS compute units of the CU numbering (default 8 when there is a peer --
        // the mask bits are dealt round-robin over the XCDs, so that is one CU per XCD; 0: no restriction), and
        // the partition levels of this context split their work over the other CUs (tc_ctx.reserved_cus).
        int cus = env_int("TC_COMM_CUS", world > 1 ? 8 : 0);
        if (cus < 0 || cus > ctx->num_cus / 4) cus = 0;
        if (cus > 0) {
            std::vector<uint32_t> mask((size_t)(ctx->num_cus + 31) / 32, 0u);
            for (int cu = ctx->num_cus - cus; cu < ctx->num_cus; cu++) mask[(size_t)cu / 32] |= 1u << (cu % 32);
            if (hipExtStreamCreateWithCUMask(&c->stream, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
                (void)hipGetLastError();
                c->stream = nullptr;
                cus = 0;
            }
        }
        if (!c->stream) TC_HIP(ctx, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->cus = cus;
        TC_HIP(ctx, hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming));
        TC_HIP(ctx, hipMalloc((void **)&c->d_words, (size_t)(1 + world) * sizeof(u64)));
        TC_HIP(ctx, hipHostMalloc((void **)&c->h_words, (size_t)(1 + world) * sizeof(u64), hipHostMallocDefault));
        RcclId u;
        memcpy(u.internal, id, TC_COMM_ID_BYTES);
        TC_NCCL(c, api->CommInitRank(&c->comm, world, u, rank));
    } catch (...) {
        comm_release(c);
        throw;
    }
    // (only a communicator that stands takes CUs away from the partition levels; the context keeps the largest
    // reservation of its live communicators)
    ctx->live_comms++;
    if (c->cus > ctx->reserved_cus) ctx->reserved_cus = c->cus;
    *out = c;
    TC_API_END(ctx)
}

void tc_comm_destroy(tc_comm *comm) {
    if (comm && comm->ctx && comm->comm) {   // (a communicator that was created: tc_comm_create counted it)
        tc_ctx *ctx = comm->ctx;
        if (ctx->live_comms > 0) ctx->live_comms--;
        if (ctx->live_comms == 0) ctx->reserved_cus = 0;
    }
    comm_release(comm);
}

int tc_comm_reserved_cus(const tc_comm *comm) { return comm ? comm->cus : 0; }

int tc_comm_wait(tc_comm *c) {
    if (!c) return TC_ERR_ARG;
    tc_ctx *ctx = c->ctx;
    TC_API_BEGIN(ctx)
    TC_HIP(ctx, hipStreamSynchronize(c->stream));
    c->inflight = false;
    TC_API_END(ctx)
}

int tc_comm_gather(tc_comm *c, int root, const uint8_t *d_container, uint64_t bytes, uint8_t *d_recv,
                   uint64_t slot_bytes, uint64_t *sizes) {
    if (!c) return TC_ERR_ARG;
    tc_ctx *ctx = c->ctx;
    TC_API_BEGIN(ctx)
    if (root < 0 || root >= c->world || !sizes || (bytes && !d_container) || (c->rank == root && !d_recv))
        TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (c->inflight) TC_FAIL(ctx, TC_ERR_ARG, "the previous gather has not been waited for");
    hipStream_t s = c->stream;
    // what the encoder produced on its stream must be there before the exchange reads it: the exchange's stream waits
    // for it on the device (no host synchronisation: the caller may already have the next record's encode queued)
    TC_HIP(ctx, hipEventRecord(c->ev_ready, ctx->stream));
    TC_HIP(ctx, hipStreamWaitEvent(s, c->ev_ready, 0));
    c->h_words[0] = bytes;
    TC_HIP(ctx, hipMemcpyAsync(c->d_words, c->h_words, sizeof(u64), hipMemcpyHostToDevice, s));
    TC_NCCL(c, c->api->AllGather(c->d_words, c->d_words + 1, 1, kNcclUint64, c->comm, s));
    TC_HIP(ctx, hipMemcpyAsync(c->h_words + 1, c->d_words + 1, (size_t)c->world * sizeof(u64), hipMemcpyDeviceToHost, s));
    TC_HIP(ctx, hipStreamSynchronize(s));
    bool over = false;
    for (int r = 0; r < c->world; r++) {
        sizes[r] = c->h_words[1 + r];
        over = over || sizes[r] > slot_bytes;
    }
    if (over) TC_FAIL(ctx, TC_ERR_CAPACITY, "a container exceeds the gather slot of %llu bytes", (unsigned long long)slot_bytes);
    TC_NCCL(c, c->api->GroupStart());
    try {
        if (c->rank == root) {
            for (int r = 0; r < c->world; r++)
                if (r != root && sizes[r])
                    TC_NCCL(c, c->api->Recv(d_recv + (size_t)r * slot_bytes, (size_t)sizes[r], kNcclUint8, r, c->comm, s));
        } else if (bytes) {
            TC_NCCL(c, c->api->Send(d_container, (size_t)bytes, kNcclUint8, root, c->comm, s));
        }
    } catch (const TcFail &) {
        (void)c->api->GroupEnd();    // never leave the thread's group open: later collectives would queue into it
        throw;
    }
    TC_NCCL(c, c->api->GroupEnd());
    if (c->rank == root && bytes)
        TC_HIP(ctx, hipMemcpyAsync(d_recv + (size_t)root * slot_bytes, d_container, bytes, hipMemcpyDeviceToDevice, s));
    c->inflight = true;
    TC_API_END(ctx)
}

int tc_comm_broadcast(tc_comm *c, int root, uint8_t *d_buf, uint64_t bytes) {
    if (!c) return TC_ERR_ARG;
    tc_ctx *ctx = c->ctx;
    TC_API_BEGIN(ctx)
    if (root < 0 || root >= c->world || (bytes && !d_buf)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) TC_NCCL(c, c->api->Broadcast(d_buf, d_buf, (size_t)bytes, kNcclUint8, root, c->comm, c->stream));
    TC_HIP(ctx, hipStreamSynchronize(c->stream));
    TC_API_END(ctx)
}

int tc_dbg_checksum64_dev(tc_ctx *ctx, const void *d_p, uint64_t bytes, uint64_t *out) {
    TC_API_BEGIN(ctx)
    if (!out || (bytes && !d_p) || (bytes & 3) || ((uintptr_t)d_p & 3)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    *out = checksum64_device(ctx, static_cast<const u8 *>(d_p), bytes);
    TC_API_END(ctx)
}

int tc_dbg_stream_bench(tc_ctx *ctx, uint64_t bytes, int width, int mode, int iters, double *gbps) {
    TC_API_BEGIN(ctx)
    if (!gbps || bytes < 4096 || iters < 1 || mode < 0 || mode > 2) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    tc_ws_reserve(ctx, 2 * bytes + 512);
    char *a = ctx->ws, *b = ctx->ws + ((bytes + 255) & ~(u64)255);
    tc_memset_async(ctx, a, 1, bytes);
    switch (width) {
        case 1: *gbps = dbg_stream_run<u8>(ctx, a, b, bytes, mode, iters); break;
        case 2: *gbps = dbg_stream_run<u16>(ctx, a, b, bytes, mode, iters); break;
        case 4: *gbps = dbg_stream_run<u32>(ctx, a, b, bytes, mode, iters); break;
        case 8: *gbps = dbg_stream_run<u64>(ctx, a, b, bytes, mode, iters); break;
        case 16: *gbps = dbg_stream_run<uint4>(ctx, a, b, bytes, mode, iters); break;
        default: TC_FAIL(ctx, TC_ERR_ARG, "width must be 1, 2, 4, 8 or 16");
    }
    TC_API_END(ctx)
}


int tc_dbg_scatter_bench(tc_ctx *ctx, uint64_t n, uint32_t bins, uint32_t xrun, int iters, double *ms_per_pass) {
    TC_API_BEGIN(ctx)
    if (!ms_per_pass || n < 4096 || n > TC_MAX_N || bins < 1 || bins > 4096 || iters < 1)
        TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    const u32 ntiles = (u32)(n / 4096);
    const u64 m = (u64)ntiles * 4096;
    u64 *k0 = nullptr, *k1 = nullptr;
    u32 *v0 = nullptr, *v1 = nullptr;
    auto carve = [&](Arena &A, bool) {
        k0 = A.get<u64>(m); k1 = A.get<u64>(m);
        v0 = A.get<u32>(m); v1 = A.get<u32>(m);
    };
    tc_ws_plan(ctx, 0, carve);
    hipStream_t s = ctx->stream;
    tc_memset_async(ctx, k0, 1, m * 8);
    tc_memset_async(ctx, v0, 1, m * 4);
    dbg_scatter_kernel<<<ntiles, 256, 0, s>>>(k0, v0, k1, v1, ntiles, bins, xrun);
    TC_LAUNCH_CHECK(ctx);
    TC_HIP(ctx, hipEventRecord(ctx->ev[6], s));
    for (int i = 0; i < iters; i++) {
        if (i & 1) dbg_scatter_kernel<<<ntiles, 256, 0, s>>>(k0, v0, k1, v1, ntiles, bins, xrun);
        else dbg_scatter_kernel<<<ntiles, 256, 0, s>>>(k1, v1, k0, v0, ntiles, bins, xrun);
    }
    TC_HIP(ctx, hipEventRecord(ctx->ev[7], s));
    TC_HIP(ctx, hipStreamSynchronize(s));
    float ms = 0;
    TC_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]));
    *ms_per_pass = ms / iters;
    TC_API_END(ctx)
}

// Where the hardware puts the workgroups of a one-per-CU grid launched on this context's stream:
// (XCC id, HW_ID, start and end of each workgroup in device clock ticks).
__global__ __launch_bounds__(1024) void dbg_dispatch_kernel(u32 *out, u32 spin) {
    extern __shared__ u32 s_big[];
    u32 hwid = 0, xcc = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const u64 t0 = __builtin_readcyclecounter();
    const u64 w0 = wall_clock64();
    s_big[threadIdx.x] = threadIdx.x;
    __syncthreads();
    u32 acc = 0;
    while (__builtin_readcyclecounter() - t0 < spin) acc += s_big[(threadIdx.x + acc) & 1023];
    const u64 w1 = wall_clock64();
    if (threadIdx.x == 0) {
        out[blockIdx.x * 6 + 0] = xcc;
        out[blockIdx.x * 6 + 1] = hwid;
        out[blockIdx.x * 6 + 2] = (u32)w0;
        out[blockIdx.x * 6 + 3] = (u32)(w0 >> 32);
        out[blockIdx.x * 6 + 4] = (u32)(w1 - w0);
        out[blockIdx.x * 6 + 5] = acc;
    }
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

int tc_dbg_dispatch_probe(tc_ctx *ctx, uint32_t grid, uint32_t lds_bytes, uint32_t spin_cycles, uint32_t *out6) {
    TC_API_BEGIN(ctx)
    if (!out6 || grid < 1 || grid > 65536 || lds_bytes < 4096 || lds_bytes > 160 * 1024) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    tc_ws_reserve(ctx, (size_t)grid * 6 * sizeof(u32) + 512);
    u32 *d = reinterpret_cast<u32 *>(ctx->ws);
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(dbg_dispatch_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    dbg_dispatch_kernel<<<grid, 1024, lds_bytes, ctx->stream>>>(d, spin_cycles);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, out6, d, (size_t)grid * 6 * sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    TC_API_END(ctx)
}

int tc_dbg_sort_bench(tc_ctx *ctx, uint64_t n, int key_bits, int iters, int check, double *ms_per_pass) {
    TC_API_BEGIN(ctx)
    if (!ms_per_pass || n < 2 || n > TC_MAX_N || key_bits < 1 || key_bits > 56 || iters < 1)
        TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    RadixBuffers b;
    u64 *src = nullptr;
    u32 *bad = nullptr;
    auto carve = [&](Arena &A, bool) {
        src = A.get<u64>(n);
        b.keys = A.get<u64>(n); b.keys_alt = A.get<u64>(n);
        b.vals = A.get<u32>(n); b.vals_alt = A.get<u32>(n);
        b.hist = A.get<u32>(RDX_MAX_PASSES * RDX_BINS);
        b.status = A.get<u64>(radix_status_words(n));
        bad = A.get<u32>(64);
    };
    tc_ws_plan(ctx, 0, carve);
    hipStream_t s = ctx->stream;
    dbg_random_keys_kernel<<<4096, 256, 0, s>>>(src, n, 0x5EEDull, key_bits);
    TC_LAUNCH_CHECK(ctx);
    RadixPlan plan;
    plan.add_range(64 - key_bits, 64);
    double total = 0;
    int launches = 0;
    const int saved = ctx->profile;
    ctx->profile = 1;
    for (int it = 0; it < iters + 1; it++) {
        RadixBuffers r = b;
        TC_HIP(ctx, hipMemcpyAsync(r.keys, src, n * sizeof(u64), hipMemcpyDeviceToDevice, s));
        ctx->pev_used = 0;
        radix_sort_pairs(ctx, r, (u32)n, plan, true, false, true);
        TC_HIP(ctx, hipStreamSynchronize(s));
        if (it > 0)
            for (int i = 0; i < ctx->pev_used; i++) {
                float ms = 0;
                TC_HIP(ctx, hipEventElapsedTime(&ms, ctx->pev[2 * i], ctx->pev[2 * i + 1]));
                total += ms;
                launches++;
            }
        if (check && it == iters) {
            tc_memset_async(ctx, bad, 0, 256);
            dbg_check_sorted_kernel<<<4096, 256, 0, s>>>(r.keys, r.vals, n, key_bits, bad);
            TC_LAUNCH_CHECK(ctx);
            tc_d2h(ctx, &ctx->h_scalars[10], bad, sizeof(u32));
            TC_HIP(ctx, hipStreamSynchronize(s));
            if ((u32)ctx->h_scalars[10]) { ctx->profile = saved; TC_FAIL(ctx, TC_ERR_INTERNAL, "sort check: %u inversions", (u32)ctx->h_scalars[10]); }
        }
    }
    ctx->profile = saved;
    *ms_per_pass = launches ? total / launches : 0;
    tc_sync_check(ctx);
    TC_API_END(ctx)
}

}  // extern "C"
