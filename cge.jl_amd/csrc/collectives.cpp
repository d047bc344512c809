// collectives.cpp -- in-library cross-GPU exchange: RCCL (the ROCm build of NCCL) over xGMI, bound at run time.
//
// One process (one cge_ctx) per GPU.  The exchange steps of the path (vect_C and the landmark-pair
// matrix of the per-edge scatter, the gathers of the sharded runsplit, the bound matrix and the scalar of the diameter) are
// all-reduces of 8-byte words; with a communicator set they are issued by the library itself on the ctx stream -- no host
// synchronisation per call, no callback into the host language, so any host (Julia, C, Python) gets them.  The caller only
// distributes the 128-byte id of rank 0 (MPI, a file, torch.distributed ...).  librccl is opened with dlopen, so the
// library loads (and single-GPU runs work) on a box whose run-time lacks librccl (the BUILD needs <rccl/rccl.h> for the
// prototypes); the hook of cge_set_collectives stays available (it is what the gloo tests on the CPU use).
// Below the RCCL binding: the exchange layer the host modules call, which chooses between the communicator and the hook.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "common.hpp"

namespace {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr; // optional (the sharded ingest of the embedding)
    decltype(&ncclReduceScatter) ReduceScatter = nullptr; // optional (the N x N landmark-pair matrix by row blocks)
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string err;
};
RcclApi &rccl() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api;
    tried = true;
    const char *names[] = {getenv("CGE_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    // A copy the process has already mapped (torch ships its own librccl) is reused: two RCCL instances in one process
    // would each bring their own topology detection and proxy threads.  Otherwise the library is loaded privately
    // (RTLD_LOCAL: its symbols must not be offered to libraries loaded later).
    for (int pass = 0; pass < 2 && !api.lib; pass++)
        for (const char *nm : names) {
            if (!nm || !*nm) continue;
            api.lib = dlopen(nm, pass == 0 ? (RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL) : (RTLD_NOW | RTLD_LOCAL));
            if (api.lib) break;
            if (pass == 1) api.err = dlerror();
        }
    if (!api.lib) return api;
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
    api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce");
    api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
    api.ReduceScatter = (decltype(api.ReduceScatter))dlsym(api.lib, "ncclReduceScatter");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) {
        api.err = "librccl lacks one of ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy";
        dlclose(api.lib);
        api.lib = nullptr;
    }
    return api;
}
const char *rccl_str(ncclResult_t r) {
    RcclApi &a = rccl();
    return a.GetErrorString ? a.GetErrorString(r) : "rccl error";
}
// the communicator's API, or the error of a context without one
RcclApi &rccl_of(cge_ctx *c) {
    RcclApi &a = rccl();
    if (!a.lib || !c->rccl_comm) CGE_THROW(CGE_E_COLLECTIVE, "no RCCL communicator on this context");
    return a;
}
// the end of every exchange: its status checked, its words counted
void rccl_done(cge_ctx *c, ncclResult_t r, const char *what, i64 words) {
    if (r != ncclSuccess) CGE_THROW(CGE_E_COLLECTIVE, "%s failed: %s", what, rccl_str(r));
    c->stat_coll_calls++;
    c->stat_coll_bytes += 8 * words;
}
// all-reduce of `count` 8-byte words in place on the ctx stream: op 0 = sum of doubles, 1 = max of doubles, 2 = sum of int64
void rccl_allreduce(cge_ctx *c, void *dev, i64 count, int op) {
    RcclApi &a = rccl_of(c);
    const ncclDataType_t dt = op == 2 ? ncclInt64 : ncclFloat64;
    const ncclRedOp_t ro = op == 1 ? ncclMax : ncclSum;
    const ncclResult_t r = a.AllReduce(dev, dev, (size_t)count, dt, ro, (ncclComm_t)c->rccl_comm, c->stream);
    rccl_done(c, r, "ncclAllReduce", count);
}

// all-gather of 8-byte words in place on the ctx stream: rank r contributes buf[r * words_per_rank, (r + 1) * words_per_rank)
// (the in-place form of ncclAllGather: sendbuff = recvbuff + rank * sendcount).  false when librccl has no ncclAllGather
// (cge_allgather_dev then falls back to a zero-filled integer all-reduce).
bool rccl_allgather(cge_ctx *c, void *dev, i64 words_per_rank) {
    RcclApi &a = rccl_of(c);
    if (!a.AllGather) return false;
    const char *mine = (const char *)dev + (size_t)8 * words_per_rank * c->coll.rank;
    const ncclResult_t r = a.AllGather(mine, dev, (size_t)words_per_rank, ncclInt64, (ncclComm_t)c->rccl_comm, c->stream);
    rccl_done(c, r, "ncclAllGather", words_per_rank * c->coll.world);
    return true;
}

// reduce-scatter (sum of doubles) in place on the ctx stream: every rank holds world * words_per_rank words; afterwards rank
// r's block [r * words_per_rank, (r + 1) * words_per_rank) holds the sums of that block over the ranks (the in-place form of
// ncclReduceScatter: recvbuff = sendbuff + rank * recvcount), the other blocks are unspecified.  A row-block reduce-scatter
// of the N x N landmark-pair matrix moves (W - 1) / W of it per link instead of the 2 (W - 1) / W of an all-reduce
// (1.9 ms vs 13 ms at N = 12000 on xGMI).  false when librccl has no ncclReduceScatter.
bool rccl_reduce_scatter(cge_ctx *c, void *dev, i64 words_per_rank) {
    RcclApi &a = rccl_of(c);
    if (!a.ReduceScatter) return false;
    char *mine = (char *)dev + (size_t)8 * words_per_rank * c->coll.rank;
    const ncclResult_t r = a.ReduceScatter(dev, mine, (size_t)words_per_rank, ncclFloat64, ncclSum, (ncclComm_t)c->rccl_comm, c->stream);
    rccl_done(c, r, "ncclReduceScatter", words_per_rank * c->coll.world);
    return true;
}
} // namespace

// ---- the exchange layer: what the host modules call ---------------------------------------------------------------------------
// With the in-library communicator an exchange is one RCCL call on the ctx stream.  The hook of cge_set_collectives works on the
// ctx exchange buffer (the host side wrapped that pointer once), on the host: a vector that lives elsewhere is copied in, the
// stream is drained, the hook runs, the result is copied back.

// One hook op through the exchange buffer.  `vec` holds `words` doubles of which [in_at, in_at + in_words) are this rank's input;
// all `words` come back.  No copies when `vec` IS the exchange buffer.
template <class Hook>
static void hook_exchange(cge_ctx *c, double *vec, i64 in_at, i64 in_words, i64 words, const char *what, Hook hook) {
    const bool copy = vec != c->xptr;
    if (copy)
        HIP_CHECK(hipMemcpyAsync(c->xptr + in_at, vec + in_at, sizeof(double) * (size_t)in_words, hipMemcpyDeviceToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (hook(c->xptr) != 0) CGE_THROW(CGE_E_COLLECTIVE, "%s hook failed", what);
    c->stat_coll_calls++;
    c->stat_coll_bytes += 8 * words;
    if (copy) HIP_CHECK(hipMemcpyAsync(vec, c->xptr, sizeof(double) * (size_t)words, hipMemcpyDeviceToDevice, c->stream));
}

bool cge_exchange_fits(cge_ctx *c, size_t need) {
    if (c->xptr && need <= c->xcap) return true;
    if (!c->rccl_comm || (c->xptr && c->xptr != c->xown.p)) return false;
    c->xown.alloc_exact(std::max<size_t>(need + need / 4, 1 << 20));
    c->xptr = c->xown.p;
    c->xcap = c->xown.n;
    return true;
}

void cge_allreduce_dev(cge_ctx *c, double *dev, i64 count, int op) {
    if (!c->has_coll) return;
    if (c->rccl_comm) { // stream-ordered, in place, no host synchronisation
        rccl_allreduce(c, dev, count, op);
        return;
    }
    // a vector that is not the exchange buffer and is longer than it goes through in pieces (an all-reduce is element-wise)
    if (!c->xptr || c->xcap == 0 || (dev == c->xptr && (size_t)count > c->xcap))
        CGE_THROW(CGE_E_COLLECTIVE, "exchange buffer too small: need %lld doubles, have %lld", (long long)count, (long long)c->xcap);
    for (i64 off = 0; off < count; off += (i64)c->xcap) {
        const i64 piece = std::min<i64>((i64)c->xcap, count - off);
        hook_exchange(c, dev + off, 0, piece, piece, "allreduce", [&](double *x) { return c->coll.allreduce_f64(c->coll.user, x, piece, op); });
    }
}

double cge_allreduce_scalar_max(cge_ctx *c, double v) {
    if (!c->has_coll) return v;
    if (!cge_exchange_fits(c, 1)) CGE_THROW(CGE_E_COLLECTIVE, "no exchange buffer set");
    HIP_CHECK(hipMemcpyAsync(c->xptr, &v, sizeof(double), hipMemcpyHostToDevice, c->stream));
    cge_allreduce_dev(c, c->xptr, 1, 1);
    HIP_CHECK(hipMemcpyAsync(&v, c->xptr, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return v;
}

// all-gather of 8-byte words in place (the sharded ingest of the embedding, the row blocks of the landmark-pair matrix):
// ncclAllGather with the in-library communicator, else the hook's own all-gather when the pieces fit the exchange buffer; with
// neither (a librccl that lacks the symbol, a hook without the op) a zero-filled all-reduce of the words as integers -- exact on
// the bit patterns (a sum of doubles would turn -0.0 into +0.0)
void cge_allgather_dev(cge_ctx *c, double *buf, i64 wpr) {
    if (!c->has_coll || wpr <= 0) return;
    if (c->rccl_comm && rccl_allgather(c, buf, wpr)) return;
    const i64 W = c->coll.world, r = c->coll.rank, total = wpr * W;
    if (!c->rccl_comm && c->coll_ext.allgather && c->xptr && (size_t)total <= c->xcap) { // (only this rank's piece goes in)
        hook_exchange(c, buf, wpr * r, wpr, total, "all-gather", [&](double *x) { return c->coll_ext.allgather(c->coll.user, x, wpr); });
        return;
    }
    if (r > 0) HIP_CHECK(hipMemsetAsync(buf, 0, sizeof(double) * (size_t)(wpr * r), c->stream));
    if (r + 1 < W) HIP_CHECK(hipMemsetAsync(buf + wpr * (r + 1), 0, sizeof(double) * (size_t)(wpr * (W - 1 - r)), c->stream));
    const i64 piece = c->rccl_comm ? total : (i64)c->xcap;
    if (piece <= 0) CGE_THROW(CGE_E_COLLECTIVE, "all-gather: no exchange buffer set");
    for (i64 off = 0; off < total; off += piece) cge_allreduce_dev(c, buf + off, std::min(piece, total - off), 2);
}

// reduce-scatter (sum of doubles) in place: `buf` holds world blocks of `wpr` words, rank r ends with the sums of block r.
// ncclReduceScatter with the in-library communicator, else the hook's reduce_scatter_f64 when the blocks fit the exchange
// buffer.  false: not available (a librccl without the symbol, a hook without the op) -- the caller all-reduces.
bool cge_reduce_scatter_dev(cge_ctx *c, double *buf, i64 wpr) {
    if (c->rccl_comm) return rccl_reduce_scatter(c, buf, wpr);
    const i64 total = wpr * c->coll.world;
    if (!c->coll_ext.reduce_scatter_f64 || !c->xptr || (size_t)total > c->xcap) return false;
    hook_exchange(c, buf, 0, total, total, "reduce-scatter", [&](double *x) { return c->coll_ext.reduce_scatter_f64(c->coll.user, x, wpr); });
    return true;
}

extern "C" {

int cge_set_collectives(cge_ctx *c, const cge_collectives *coll) {
    if (!c) return CGE_E_ARG;
    c->has_coll = coll && coll->allreduce_f64 && coll->world > 1;
    if (c->has_coll) c->coll = *coll;
    c->coll_ext = cge_collectives_ext{};
    return CGE_OK;
}
int cge_set_collectives_ext(cge_ctx *c, const cge_collectives_ext *ext) {
    if (!c) return CGE_E_ARG;
    c->coll_ext = ext ? *ext : cge_collectives_ext{};
    return CGE_OK;
}

int cge_exchange_buffer(cge_ctx *c, int64_t min_doubles, void **dev_ptr, int64_t *cap) {
    if (!c) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if ((size_t)min_doubles > c->xown.n || !c->xown.p) c->xown.alloc_exact((size_t)std::max<i64>(min_doubles, 1024));
    c->xptr = c->xown.p;
    c->xcap = c->xown.n;
    if (dev_ptr) *dev_ptr = c->xptr;
    if (cap) *cap = (int64_t)c->xcap;
    CGE_CATCH(c)
}

int cge_set_exchange_buffer(cge_ctx *c, void *dev_ptr, int64_t cap) {
    if (!c || !dev_ptr || cap < 1) return CGE_E_ARG;
    c->xptr = (double *)dev_ptr;
    c->xcap = (size_t)cap;
    return CGE_OK;
}

int cge_rccl_unique_id(void *id_out) {
    if (!id_out) return CGE_E_ARG;
    RcclApi &a = rccl();
    if (!a.lib) return CGE_E_COLLECTIVE;
    static_assert(sizeof(ncclUniqueId) == CGE_RCCL_ID_BYTES, "cge_hip.h: CGE_RCCL_ID_BYTES");
    ncclUniqueId id;
    if (a.GetUniqueId(&id) != ncclSuccess) return CGE_E_COLLECTIVE;
    memcpy(id_out, &id, sizeof(id));
    return CGE_OK;
}

int cge_comm_init_rccl(cge_ctx *c, const void *id_in, int rank, int world) {
    if (!c || !id_in || world < 1 || rank < 0 || rank >= world) return CGE_E_ARG;
    CGE_TRY(c)
    RcclApi &a = rccl();
    if (!a.lib) CGE_THROW(CGE_E_COLLECTIVE, "librccl could not be opened: %s", a.err.c_str());
    HIP_CHECK(hipSetDevice(c->device));
    if (c->rccl_comm) { (void)a.CommDestroy((ncclComm_t)c->rccl_comm); c->rccl_comm = nullptr; }
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof(id));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = a.CommInitRank(&comm, world, id, rank);
    if (r != ncclSuccess) CGE_THROW(CGE_E_COLLECTIVE, "ncclCommInitRank(rank %d of %d) failed: %s", rank, world, rccl_str(r));
    c->rccl_comm = comm;
    c->coll.allreduce_f64 = nullptr;
    c->coll.user = nullptr;
    c->coll.rank = rank;
    c->coll.world = world;
    c->has_coll = world > 1; // a one-rank communicator is legal (self test) but shards nothing
    CGE_CATCH(c)
}

int cge_comm_finalize(cge_ctx *c) {
    if (!c) return CGE_E_ARG;
    if (c->rccl_comm) {
        (void)hipStreamSynchronize(c->stream);
        RcclApi &a = rccl();
        if (a.lib) (void)a.CommDestroy((ncclComm_t)c->rccl_comm);
        c->rccl_comm = nullptr;
        c->has_coll = false;
    }
    return CGE_OK;
}

// testing hook (include/cge_hip_testing.h): host array -> device -> in-library all-reduce -> host
int cge_rccl_selftest(void *ctx, double *host_inout, int64_t count, int op) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !host_inout || count <= 0) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    DevBuf<double> d;
    d.ensure((size_t)count);
    HIP_CHECK(hipMemcpyAsync(d.p, host_inout, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    rccl_allreduce(c, d.p, count, op);
    HIP_CHECK(hipMemcpyAsync(host_inout, d.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CGE_CATCH(c)
}

} // extern "C"
