// tc_comm.hpp -- the one exchange of the multi-GPU path behind the C ABI: records are
// independent, one per GPU, nothing is exchanged during the encode; at the end the variable-size
// containers are gathered on one rank -- sizes by an all-gather of one word per rank, then ONE group in
// which the root posts a receive per peer and every peer one send, so that the root ingests on all of its
// xGMI links at once (a ring would be bound by a single link) -- and an FM-index is replicated by one
// broadcast.  The reference has no counterpart: its only parallelism is parListChunk over the pattern
// list inside one process (FMIndex.hs:417-423).
//
// RCCL is bound at run time (dlopen; the copy the process has already loaded, e.g. PyTorch's, is
// preferred), so libtextcomp.so itself does not depend on it: a single-GPU user never loads it, and a
// missing / failing RCCL is the status code TC_ERR_NCCL, not a load error.
#pragma once
#include <dlfcn.h>
#include <stdlib.h>

#include <mutex>

#include "tc_common.hpp"

struct RcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, /* ncclUniqueId by value */ struct RcclId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
struct RcclId {
    char internal[TC_COMM_ID_BYTES];   // = ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128)
};
enum { kNcclUint8 = 1, kNcclUint64 = 5 };   // ncclDataType_t

// TC_RCCL_LIB (tests, unusual installs): the one library name to bind instead of the list below.
static RcclApi *rccl_api(std::string *why) {
    static RcclApi api;
    static std::string err;
    static std::once_flag once;      // tc_comm_* may be entered from several contexts / threads at once
    std::call_once(once, [] {
        const char *only = getenv("TC_RCCL_LIB");
        const char *dflt[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
        std::vector<const char *> names;
        if (only && *only) names.push_back(only);
        else names.assign(dflt, dflt + 3);
        for (const char *n : names)
            if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);   // a copy already in the process
        for (const char *n : names)
            if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!api.lib) {
            const char *e = dlerror();    // (one call: dlerror() clears the message it returns)
            err = std::string("librccl not found: ") + (e ? e : "?");
            return;
        }
        auto sym = [&](const char *s) {
            void *p = dlsym(api.lib, s);
            if (!p && err.empty()) err = std::string("librccl lacks ") + s;
            return p;
        };
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
        api.Broadcast = reinterpret_cast<decltype(api.Broadcast)>(sym("ncclBroadcast"));
        api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
        api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
        api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    });
    if (!err.empty()) {
        if (why) *why = err;
        return nullptr;
    }
    return &api;
}

struct tc_comm {
    tc_ctx *ctx = nullptr;
    RcclApi *api = nullptr;
    void *comm = nullptr;
    int rank = 0, world = 1;
    hipStream_t stream = nullptr;   // the exchange runs beside the encoder's stream
    hipEvent_t ev_ready = nullptr;  // recorded on the encoder's stream when a gather is posted: the exchange waits for it on the device
    u64 *d_words = nullptr;         // [1 + world] my size, all sizes
    u64 *h_words = nullptr;         // pinned mirror
    bool inflight = false;
    int cus = 0;                    // compute units the exchange is restricted to (0: any)
};

#define TC_NCCL(c, expr)                                                                         \
    do {                                                                                         \
        int r__ = (expr);                                                                        \
        if (r__ != 0) {                                                                          \
            char b__[512];                                                                       \
            snprintf(b__, sizeof b__, "%s -> %s", #expr, (c)->api->GetErrorString(r__));         \
            (c)->ctx->err = b__;                                                                 \
            throw TcFail{TC_ERR_NCCL};                                                           \
        }                                                                                        \
    } while (0)

static void comm_release(tc_comm *c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && c->api) (void)c->api->CommDestroy(c->comm);
    if (c->d_words) (void)hipFree(c->d_words);
    if (c->h_words) (void)hipHostFree(c->h_words);
    if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// ---- the bodies of the tc_comm_* entry points (textcomp.hip forwards to them inside TC_API_BEGIN / TC_API_END)
static void comm_unique_id_entry(tc_ctx *ctx, u8 *id) {
    if (!id) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    std::string why;
    RcclApi *api = rccl_api(&why);
    if (!api) TC_FAIL(ctx, TC_ERR_NCCL, "%s", why.c_str());
    RcclId u;
    const int r = api->GetUniqueId(&u);
    if (r != 0) TC_FAIL(ctx, TC_ERR_NCCL, "ncclGetUniqueId -> %s", api->GetErrorString(r));
    memcpy(id, u.internal, TC_COMM_ID_BYTES);
}
static void comm_create_entry(tc_ctx *ctx, const u8 *id, int rank, int world, tc_comm **out) {
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
}
static void comm_destroy_entry(tc_comm *comm) {
    if (comm && comm->ctx && comm->comm) {   // (a communicator that was created: tc_comm_create counted it)
        tc_ctx *ctx = comm->ctx;
        if (ctx->live_comms > 0) ctx->live_comms--;
        if (ctx->live_comms == 0) ctx->reserved_cus = 0;
    }
    comm_release(comm);
}
static void comm_wait_entry(tc_ctx *ctx, tc_comm *c) {
    TC_HIP(ctx, hipStreamSynchronize(c->stream));
    c->inflight = false;
}
static void comm_gather_entry(tc_ctx *ctx, tc_comm *c, int root, const u8 *d_container, u64 bytes, u8 *d_recv, u64 slot_bytes,
                              u64 *sizes) {
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
}
static void comm_broadcast_entry(tc_ctx *ctx, tc_comm *c, int root, u8 *d_buf, u64 bytes) {
    if (root < 0 || root >= c->world || (bytes && !d_buf)) TC_FAIL(ctx, TC_ERR_ARG, "bad argument");
    TC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) TC_NCCL(c, c->api->Broadcast(d_buf, d_buf, (size_t)bytes, kNcclUint8, root, c->comm, c->stream));
    TC_HIP(ctx, hipStreamSynchronize(c->stream));
}
