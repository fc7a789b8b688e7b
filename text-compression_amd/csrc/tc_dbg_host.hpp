// tc_dbg_host.hpp -- the calibration and debug interface (include/textcomp_debug.h): the kernels that measure the memory
// system without any of the pipeline's work, and the bodies of the tc_dbg_* calls.  Included by textcomp.hip only, after
// tc_container_host.hpp (checksum64_device), tc_encode_host.hpp (seg_sort_pairs, seg_carve) and tc_ws_host.hpp.
#pragma once
#include "tc_container_host.hpp"
#include "tc_encode_host.hpp"
#include "tc_radix_host.hpp"

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

// Where the hardware puts the workgroups of a one-per-CU grid launched on this context's stream:
// (XCC id, HW_ID, start and end of each workgroup in device clock ticks).
extern "C" __global__ __launch_bounds__(1024) void dbg_dispatch_kernel(u32 *out, u32 spin) {   // (C linkage: the name it has in traces)
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

static void dbg_checksum64_entry(tc_ctx *ctx, const void *d_p, u64 bytes, u64 *out) {
    if (!out || (bytes && !d_p) || (bytes & 3) || ((uintptr_t)d_p & 3)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    *out = checksum64_device(ctx, static_cast<const u8 *>(d_p), bytes);
}
static void dbg_stream_bench_entry(tc_ctx *ctx, u64 bytes, int width, int mode, int iters, double *gbps) {
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
}
static void dbg_scatter_bench_entry(tc_ctx *ctx, u64 n, u32 bins, u32 xrun, int iters, double *ms_per_pass) {
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
}
static void dbg_dispatch_probe_entry(tc_ctx *ctx, u32 grid, u32 lds_bytes, u32 spin_cycles, u32 *out6) {
    if (!out6 || grid < 1 || grid > 65536 || lds_bytes < 4096 || lds_bytes > 160 * 1024) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    tc_ws_reserve(ctx, (size_t)grid * 6 * sizeof(u32) + 512);
    u32 *d = reinterpret_cast<u32 *>(ctx->ws);
    TC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(dbg_dispatch_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    dbg_dispatch_kernel<<<grid, 1024, lds_bytes, ctx->stream>>>(d, spin_cycles);
    TC_LAUNCH_CHECK(ctx);
    tc_d2h(ctx, out6, d, (size_t)grid * 6 * sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
}
static void dbg_sort_bench_entry(tc_ctx *ctx, u64 n, int key_bits, int iters, int check, double *ms_per_pass) {
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
}

// ------------------------------------------------------------ the segmented sort and the one-workgroup network on the caller's data
// tc_dbg_seg_sort: seg_sort_pairs (tc_sa_host.hpp) as a doubling round calls it, on pairs staged through the workspace,
// with the tables a text of m suffixes gets (seg_carve).  No kernel of its own.
static void dbg_seg_sort_entry(tc_ctx *ctx, u64 *keys, u32 *vals, u32 m, int rbits, u32 *levels) {
    if (!keys || !vals || !levels || m < 1 || m > (1u << 24) || rbits < 1 || rbits > 32) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    for (u32 i = 0; i < m; i++) {
        if (i && (keys[i] >> 32) < (keys[i - 1] >> 32)) TC_FAIL(ctx, TC_ERR_ARG, "grp decreases at member %u", i);
        if (rbits < 32 && ((u32)keys[i] >> rbits) != 0) TC_FAIL(ctx, TC_ERR_ARG, "rank of member %u has more than %d bits", i, rbits);
    }
    SegBuffers g;
    u64 *kx = nullptr, *ky = nullptr;
    u32 *vx = nullptr, *vy = nullptr;
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        kx = A.get<u64>(m); ky = A.get<u64>(m);
        vx = A.get<u32>(m); vy = A.get<u32>(m);
        seg_carve(A, m, g);
    });
    tc_h2d(ctx, kx, keys, (size_t)m * sizeof(u64));
    tc_h2d(ctx, vx, vals, (size_t)m * sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    seg_sort_pairs(ctx, g, kx, vx, ky, vy, m, rbits, levels);
    tc_d2h(ctx, keys, kx, (size_t)m * sizeof(u64));
    tc_d2h(ctx, vals, vx, (size_t)m * sizeof(u32));
    tc_sync_check(ctx);
}
// tc_dbg_tied_small: tied_small_kernel<mode> (tc_seg.hpp) as sa_order_tied (mode 0) and the sparse rank table (mode 1) launch it
static void dbg_tied_small_entry(tc_ctx *ctx, int mode, u32 *slot, u32 *idx, u32 *grp, u32 m, u32 *t_idx, u32 *t_rank, u32 *tpos) {
    if ((mode != 0 && mode != 1) || !slot || !idx || !grp || m < 1 || m > SEG_W) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    if (mode == 1 && (!t_idx || !t_rank || !tpos)) TC_FAIL(ctx, TC_ERR_ARG, "mode 1 needs t_idx, t_rank and tpos");
    u32 *d[6] = {};
    tc_ws_plan(ctx, 0, [&](Arena &A, bool) {
        for (int q = 0; q < 6; q++) d[q] = A.get<u32>(m);
    });
    u32 *const h_in[3] = {slot, idx, grp};
    for (int q = 0; q < 3; q++) tc_h2d(ctx, d[q], h_in[q], (size_t)m * sizeof(u32));
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (mode == 0) tied_small_kernel<0><<<1, SEG_NT, 0, ctx->stream>>>(d[0], d[1], d[2], m, nullptr, nullptr, nullptr);
    else tied_small_kernel<1><<<1, SEG_NT, 0, ctx->stream>>>(d[0], d[1], d[2], m, d[3], d[4], d[5]);
    TC_LAUNCH_CHECK(ctx);
    u32 *const h_out[3] = {mode == 0 ? slot : t_idx, mode == 0 ? idx : t_rank, mode == 0 ? grp : tpos};
    for (int q = 0; q < 3; q++) tc_d2h(ctx, h_out[q], d[mode == 0 ? q : 3 + q], (size_t)m * sizeof(u32));
    tc_sync_check(ctx);
}
