// tc_ws_host.hpp -- the context's device workspace: one hipMalloc block, or physical chunks mapped into one reserved
// address range that grows in place; tc_ws_reserve (every stage's tc_ws_plan ends here), the chunked allocation other
// stages borrow (tc_chunked_alloc), the grid size of the persistent kernels, the check of the device error word, and
// the body of tc_ctx_place_workspace.  Included by textcomp.hip only, after tc_encode_host.hpp (encode_device).
#pragma once
#include <chrono>
#include <vector>

#include "tc_encode_host.hpp"

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

// tc_ctx_place_workspace: the record is encoded on up to `tries` placements of the workspace, the fastest stays
static void ws_place_entry(tc_ctx *ctx, const u8 *d_text, u64 n, tc_block *out, int tries, double *ms, int *chosen) {
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
}
