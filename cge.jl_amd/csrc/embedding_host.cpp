// embedding_host.cpp -- everything that makes an embedding resident: the row-major fp64 matrix Xr of the context, whole, or the rows
// of this rank's communities (option shard_rows).
//
// ONE INGEST takes a cge_embedding_view (include/cge_hip.h: fp64 / fp32 / fp16 / bf16, host or device, either layout, any leading
// dimension) in four stages over one small record: check -> place (which rows this rank keeps, where they land) -> bring (fill
// them) -> finish.  The fp64 entry points cge_set_embedding / cge_set_embedding_device describe their matrix as a view and call it.
// A host view travels in its own type -- raw bytes through the pinned staging buffers -- and is widened on the device
// (kernels_ingest.hip) behind each chunk; widening is exact and an fp64 "widening" is a copy ("Embedding views").
#include <cmath>

#include "common.hpp"

bool ingest_sharded(const cge_ctx *c) { return c->opt_shard_ingest && c->has_coll && c->coll.world > 1; }

// ---- option "shard_rows": the embedding rows sharded by community (common.hpp) ---------------------------------------------
static bool rows_shard_wanted(const cge_ctx *c) { return c->opt_shard_rows && c->has_coll && c->coll.world > 1; }
void rows_unshard(cge_ctx *c) {
    c->rows_sharded = false;
    c->n_loc = 0;
    c->h_loc2glob.clear(); c->h_glob2loc.clear(); c->comm_owner.clear(); c->h_vw_loc.clear();
    c->loc2glob.release(); c->glob2loc.release(); c->comm_loc.release(); c->vw_loc.release();
}
// local copies of the per-vertex tables the row passes read (weights, communities of this rank's rows)
void rows_refresh_local_tables(cge_ctx *c) {
    if (!c->rows_sharded) return;
    const i64 nl = c->n_loc;
    if ((i64)c->h_vw.size() == c->n) {
        c->h_vw_loc.resize(nl);
        for (i64 i = 0; i < nl; i++) c->h_vw_loc[i] = c->h_vw[c->h_loc2glob[i]];
        c->vw_loc.alloc_exact(nl);
        HIP_CHECK(hipMemcpyAsync(c->vw_loc.p, c->h_vw_loc.data(), sizeof(double) * nl, hipMemcpyHostToDevice, c->stream));
    }
    std::vector<i32> cl(nl);
    for (i64 i = 0; i < nl; i++) cl[i] = c->h_comm[c->h_loc2glob[i]];
    c->comm_loc.alloc_exact(nl);
    HIP_CHECK(hipMemcpyAsync(c->comm_loc.p, cl.data(), sizeof(i32) * nl, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
// THE OWNERSHIP RULE (the same on every rank: it reads the replicated community vector only): communities by decreasing
// size (ties: lower id first), each to the rank with the fewest rows so far (ties: lower rank).  cge.jl_amd/dist.py
// restates it (community_owner) and tests/test_distributed_gloo.py holds the two together.
static void rows_assign_ownership(cge_ctx *c) {
    const i64 n = c->n, C = c->n_comm_max, W = c->coll.world;
    if ((i64)c->h_comm.size() != n || C <= 0)
        CGE_THROW(CGE_E_ARG, "option shard_rows: upload the communities (cge_set_vertex_data) before the embedding -- the rows are sharded by community");
    std::vector<i64> size(C, 0), ord(C), load(W, 0);
    for (i64 i = 0; i < n; i++) size[c->h_comm[i]]++;
    for (i64 q = 0; q < C; q++) ord[q] = q;
    std::stable_sort(ord.begin(), ord.end(), [&](i64 a, i64 b) { return size[a] > size[b]; });
    c->comm_owner.assign(C, 0);
    for (i64 q : ord) {
        const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        c->comm_owner[q] = r;
        load[r] += size[q];
    }
    // A rank without a row cannot take part; EVERY rank refuses then (the loads are the same on every rank), so that no rank
    // goes on into the all-reduce of the column sums while another has left with an error.  Nothing stays resident.
    const int starved = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    if (load[starved] <= 0) {
        c->Xr.release(); c->h_Xr.clear();
        c->d = 0;
        rows_unshard(c);
        CGE_THROW(CGE_E_ARG, "option shard_rows: fewer communities than ranks (rank %d would own no row)", starved);
    }
    const int me = c->coll.rank;
    c->h_glob2loc.assign(n, -1);
    c->h_loc2glob.clear();
    c->h_loc2glob.reserve(load[me]);
    for (i64 i = 0; i < n; i++)
        if (c->comm_owner[c->h_comm[i]] == me) {
            c->h_glob2loc[i] = (i32)c->h_loc2glob.size();
            c->h_loc2glob.push_back((i32)i);
        }
    c->n_loc = (i64)c->h_loc2glob.size();
    c->loc2glob.alloc_exact(c->n_loc);
    c->glob2loc.alloc_exact(n);
    HIP_CHECK(hipMemcpyAsync(c->loc2glob.p, c->h_loc2glob.data(), sizeof(i32) * c->n_loc, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(c->glob2loc.p, c->h_glob2loc.data(), sizeof(i32) * n, hipMemcpyHostToDevice, c->stream));
    c->rows_sharded = true;
    rows_refresh_local_tables(c);
}

// host mirror of the row-major embedding: only the generic round-based rss path (ties at the maximum of z, NaNs) and the
// exact unique-row count read it, so it is fetched on first demand instead of at every upload (1 GB at the headline)
void cge_ensure_host_embedding(cge_ctx *c) {
    const size_t need = (size_t)lm_rows(c) * (size_t)c->d; // (option shard_rows: this rank's rows, local ids)
    if (c->h_Xr.size() == need) return;
    if (!c->Xr.p || need == 0) CGE_THROW(CGE_E_ARG, "embedding not resident");
    c->h_Xr.resize(need);
    HIP_CHECK(hipMemcpyAsync(c->h_Xr.data(), c->Xr.p, sizeof(double) * need, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// what every upload ends with: sizes, the global feature mean (the centre of the diameter kernels' operands).  The centred
// feature-major copy of the brute-force diameter kernel is built on first use (it is as large as the embedding and the pruned
// path never reads it).
static void embedding_resident(cge_ctx *c, i64 n, i64 d) {
    c->h_Xr.clear();
    c->h_Xr.shrink_to_fit();
    c->n = n;
    c->d = d;
    c->ldn = (n + 127) / 128 * 128;
    c->dpad = (d + 15) / 16 * 16;
    c->Xc.release();
    c->rnorm.release();
    c->gmean.alloc_exact((size_t)d);
    if (c->rows_sharded) { // column sums of the local rows, added over the ranks (every rank ends with the same bits), / n
        k_col_mean(c, c->Xr.p, c->n_loc, d, c->gmean.p, 1.0);
        cge_allreduce_dev(c, c->gmean.p, d, 0);
        k_scale_vector(c, c->gmean.p, d, 1.0 / (double)n);
    } else
        k_col_mean(c, c->Xr.p, n, d, c->gmean.p);
    // A NaN or an Inf anywhere in the embedding reaches its column's mean.  The reference's `hi` is then NaN (extrema() over
    // distances that hold a NaN, src/divergence.jl:113), and the diameter entry points answer that instead of the maximum over
    // the pairs that happen to compare: a comparison with NaN is false, so the tile kernels would skip those pairs silently.
    std::vector<double> hmean(d);
    HIP_CHECK(hipMemcpyAsync(hmean.data(), c->gmean.p, sizeof(double) * d, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->emb_nonfinite = false;
    for (double m : hmean) c->emb_nonfinite |= !std::isfinite(m);
    c->centred_ready = false;
    c->lm_ready = false;
}

// ---- the boundary checks of a view ------------------------------------------------------------------------------------------------
int view_check(const cge_embedding_view *v, i64 n, std::string &msg) {
    char b[256];
    b[0] = 0;
    if (!v) snprintf(b, sizeof b, "embedding view: NULL view");
    else if (!v->data) snprintf(b, sizeof b, "embedding view: NULL data");
    else if (n <= 0 || v->d <= 0) snprintf(b, sizeof b, "embedding view: n = %lld, d = %lld (both must be positive)", (long long)n, (long long)v->d);
    else if (v->dtype < CGE_DTYPE_F64 || v->dtype > CGE_DTYPE_BF16) snprintf(b, sizeof b, "embedding view: unknown dtype %d", v->dtype);
    else if (v->ld < 0 || (v->ld != 0 && v->ld < (v->row_major ? v->d : n)))
        snprintf(b, sizeof b, "embedding view: leading dimension %lld below the packed %lld", (long long)v->ld, (long long)(v->row_major ? v->d : n));
    else if ((uintptr_t)v->data % cge_dtype_size(v->dtype) != 0)
        snprintf(b, sizeof b, "embedding view: data pointer not aligned to its %d-byte elements", (int)cge_dtype_size(v->dtype));
    else return CGE_OK;
    msg = b;
    return CGE_E_ARG;
}
// the kernels dereference the pointer on the context's GPU: host memory and another GPU's memory are refused (nothing is read)
void check_device_pointer(const cge_ctx *c, const char *who, const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        CGE_THROW(CGE_E_ARG, "%s: the pointer is not device memory", who);
    }
    if (at.device != c->device)
        CGE_THROW(CGE_E_ARG, "%s: the pointer lies on GPU %d, the context is on GPU %d", who, at.device, c->device);
}

// ---- the ingest -------------------------------------------------------------------------------------------------------------------
struct Ingest {
    cge_ctx *c;
    const char *who;             // the entry point that was called, for messages
    const cge_embedding_view *v;
    const i64 n;
    i64 d = 0, ld = 0;           // ld: in elements, the packed value filled in
    int dt = 0;
    bool rm = false;
    size_t es = 0, pitch = 0;    // bytes of an element, of a step of the leading dimension
    // place: this rank brings `nl` rows to `dst` (in Xr) -- rows [r0, r0 + nl) of the caller's matrix, or the listed ones
    i64 nl = 0, r0 = 0;
    double *dst = nullptr;
    const i32 *h_idx = nullptr, *d_idx = nullptr; // option shard_rows: the rows of this rank's communities (host and device list)
    i64 per = 0;                 // option shard_ingest: the rows of a rank's slice (the slices are all-gathered), else 0
    DevBuf<unsigned char> raw;   // the typed image on the device: this rank's packed rows, or a ring of two chunks
};

static void ingest_check(Ingest &S) {
    cge_ctx *c = S.c;
    const cge_embedding_view *v = S.v;
    std::string msg;
    if (view_check(v, S.n, msg) != CGE_OK) CGE_THROW(CGE_E_ARG, "%s", msg.c_str());
    HIP_CHECK(hipSetDevice(c->device));
    if (c->n && c->n != S.n) CGE_THROW(CGE_E_ASSERT, "No. rows in embedding and no. vertices in a graph differ.");
    if (v->on_device) check_device_pointer(c, S.who, v->data);
    S.d = v->d;
    S.dt = v->dtype;
    S.rm = v->row_major != 0;
    S.ld = v->ld ? v->ld : (S.rm ? S.d : S.n);
    S.es = cge_dtype_size(S.dt);
    S.pitch = (size_t)S.ld * S.es;
}

// Which rows this rank keeps and where they land.  Option shard_rows: the rows of its own communities only (n / world rows over
// its own PCIe link, nothing over xGMI).  Option shard_ingest (host views): every rank uploads n / world ROWS over its own link
// into its place of Xr and the pieces are all-gathered device to device -- instead of world full uploads side by side; equal
// pieces of `per` rows (ncclAllGather), so Xr carries up to world - 1 rows of zero padding behind row n.  Else all n rows.
static void ingest_place(Ingest &S) {
    cge_ctx *c = S.c;
    const i64 n = S.n, d = S.d;
    if (rows_shard_wanted(c)) {
        rows_assign_ownership(c);
        S.nl = c->n_loc;
        S.h_idx = c->h_loc2glob.data();
        S.d_idx = c->loc2glob.p;
        c->Xr.alloc_exact((size_t)S.nl * d);
        S.dst = c->Xr.p;
        return;
    }
    rows_unshard(c);
    if (ingest_sharded(c) && !S.v->on_device) {
        const i64 W = c->coll.world, r = c->coll.rank, per = (n + W - 1) / W;
        S.per = per;
        S.r0 = std::min<i64>(n, per * r);
        S.nl = std::min<i64>(n, S.r0 + per) - S.r0;
        c->Xr.alloc_exact((size_t)per * W * d);
        S.dst = c->Xr.p + (size_t)per * r * d;
        if (S.nl < per) HIP_CHECK(hipMemsetAsync(S.dst + (size_t)S.nl * d, 0, sizeof(double) * (size_t)(per - S.nl) * d, c->stream));
        return;
    }
    S.nl = n;
    c->Xr.alloc_exact((size_t)n * d);
    S.dst = c->Xr.p;
}

// a device view: one pass over the caller's matrix
static void bring_device(Ingest &S) {
    cge_ctx *c = S.c;
    const void *X = S.v->data;
    if (S.d_idx) k_ingest_gather(c, X, S.dt, S.ld, S.d, S.rm, S.d_idx, S.nl, S.dst);
    else if (S.rm && S.dt == CGE_DTYPE_F64 && S.ld == S.d)
        HIP_CHECK(hipMemcpyAsync(S.dst, X, sizeof(double) * (size_t)S.n * S.d, hipMemcpyDeviceToDevice, c->stream));
    else if (S.rm) k_ingest_rows(c, X, S.dt, S.ld, S.n, S.d, S.dst);
    else k_ingest_cols(c, X, S.dt, S.ld, S.dst, S.n, S.d, 0, 0, S.d);
}

// bytes [a0, a1) of a packed image made of runs of `run` bytes, run j starting at base + (idx ? idx[j] : j) * pitch
static void copy_runs(unsigned char *o, size_t a0, size_t a1, const unsigned char *base, size_t run, size_t pitch, const i32 *idx) {
    if (!idx && run == pitch) { memcpy(o, base + a0, a1 - a0); return; }
    for (size_t e = a0; e < a1;) {
        const size_t j = e / run, at = e % run, len = std::min(a1 - e, run - at);
        memcpy(o + (e - a0), base + (idx ? (size_t)idx[j] : j) * pitch + at, len);
        e += len;
    }
}
// listed rows of a column-major host view, packed: element e of the (nl x d, column-major) image is column e / nl, row idx[e % nl]
// -- a gather of single elements, typed by their size
template <typename U>
static void upload_gathered_cols(Ingest &S) {
    const U *X = (const U *)S.v->data;
    const size_t nl = (size_t)S.nl, ld = (size_t)S.ld;
    const i32 *idx = S.h_idx;
    staged_upload<U>(S.c, (U *)S.raw.p, nl * (size_t)S.d, [=](U *o, size_t a0, size_t a1) {
        size_t k = a0 / nl, i = a0 % nl;
        for (size_t e = a0; e < a1; e++) {
            o[e - a0] = X[k * ld + (size_t)idx[i]];
            if (++i == nl) { i = 0; k++; }
        }
    });
}
// a host view under either sharding: a packed typed image of the placed rows (row-major: rows of d; column-major: columns of nl)
// goes up whole and is widened into their place
static void bring_packed(Ingest &S) {
    cge_ctx *c = S.c;
    const i64 nl = S.nl, d = S.d;
    if (nl <= 0) return;
    const size_t es = S.es, pitch = S.pitch, total = (size_t)nl * d * es;
    S.raw.alloc_exact(total);
    if (!S.rm && S.h_idx) {
        if (es == 8) upload_gathered_cols<uint64_t>(S);
        else if (es == 4) upload_gathered_cols<uint32_t>(S);
        else upload_gathered_cols<uint16_t>(S);
    } else { // whole rows of a row-major view (listed, or a run of them); rows [r0, r0 + nl) of every column of a column-major one
        const unsigned char *base = (const unsigned char *)S.v->data + (size_t)S.r0 * (S.rm ? pitch : es);
        const size_t run = (size_t)(S.rm ? d : nl) * es;
        const i32 *idx = S.h_idx;
        staged_upload<unsigned char>(c, S.raw.p, total, [=](unsigned char *o, size_t a0, size_t a1) { copy_runs(o, a0, a1, base, run, pitch, idx); });
    }
    if (S.rm) k_ingest_rows(c, S.raw.p, S.dt, d, nl, d, S.dst);
    else k_ingest_cols(c, S.raw.p, S.dt, nl, S.dst, nl, d, 0, 0, d);
}

// A whole host view: it goes up in chunks through a ring of two chunks on the device; every chunk is widened (and transposed) into
// its place of Xr right behind its copy, on the stream, while the next chunk is on the wire: no n x d typed device buffer, no
// separate pass over it.
static void bring_ring(Ingest &S) {
    cge_ctx *c = S.c;
    const unsigned char *X = (const unsigned char *)S.v->data;
    const i64 n = S.n, d = S.d;
    const int dt = S.dt;
    const size_t es = S.es, pitch = S.pitch, cap = CGE_STAGE_BYTES, total = (size_t)n * d * es;
    double *Xr = S.dst;
    if (S.rm) {
        // row-major: the packed image has Xr's own order, so a chunk is any run of elements (a multiple of 16 bytes: the ring slots
        // and the chunk's place in Xr stay aligned for the vector loads and stores) and is widened in place behind its copy
        const size_t chunk = std::min(cap, std::max((size_t)2 << 20, ((total + 7) / 8 + 15) / 16 * 16));
        S.raw.alloc_exact(2 * chunk);
        staged_upload_chunks<unsigned char>(
            c, S.raw.p, total, chunk, 2, [=](unsigned char *o, size_t a0, size_t a1) { copy_runs(o, a0, a1, X, (size_t)d * es, pitch, nullptr); },
            [=](unsigned char *piece, size_t off, size_t len) { k_ingest_rows(c, piece, dt, (i64)(len / es), 1, (i64)(len / es), Xr + off / es); });
    } else if ((size_t)n * es <= cap) { // column-major: chunks of whole columns
        const size_t colb = (size_t)n * es, kc = std::min<size_t>((size_t)d, cap / colb), chunk = kc * colb;
        S.raw.alloc_exact(2 * chunk);
        staged_upload_chunks<unsigned char>(
            c, S.raw.p, total, chunk, 2, [=](unsigned char *o, size_t a0, size_t a1) { copy_runs(o, a0, a1, X, colb, pitch, nullptr); },
            [=](unsigned char *piece, size_t off, size_t len) { k_ingest_cols(c, piece, dt, n, Xr, n, (i64)(len / colb), 0, (i64)(off / colb), d); });
    } else { // a column longer than a staging buffer: one column at a time, in row pieces
        S.raw.alloc_exact(2 * cap);
        for (i64 k = 0; k < d; k++)
            staged_upload_chunks<unsigned char>(
                c, S.raw.p, (size_t)n * es, cap, 2, [=](unsigned char *o, size_t a0, size_t a1) { memcpy(o, X + (size_t)k * pitch + a0, a1 - a0); },
                [=](unsigned char *piece, size_t off, size_t len) { k_ingest_cols(c, piece, dt, (i64)(len / es), Xr, (i64)(len / es), 1, (i64)(off / es), k, d); });
    }
}

static void ingest_finish(Ingest &S) {
    cge_ctx *c = S.c;
    if (S.per) cge_allgather_dev(c, c->Xr.p, S.per * S.d);
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (a device view: the caller may free or reuse its buffer on return)
    S.raw.release();
    embedding_resident(c, S.n, S.d);
}

void set_embedding_view(cge_ctx *c, const char *who, const cge_embedding_view *v, i64 n) {
    Ingest S{c, who, v, n};
    link_drop(c); // (a link model refers to the resident embedding)
    ingest_check(S);
    ingest_place(S);
    if (v->on_device) bring_device(S);
    else if (S.h_idx || S.per) bring_packed(S);
    else bring_ring(S);
    ingest_finish(S);
}

extern "C" {

int cge_embedding_view_check(const cge_embedding_view *v, int64_t n, char *err, int64_t err_len) {
    std::string msg;
    const int rc = view_check(v, n, msg);
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg.c_str());
    return rc;
}

int cge_set_embedding_view(cge_ctx *c, const cge_embedding_view *v, int64_t n) {
    if (!c || !v) return CGE_E_ARG;
    CGE_TRY(c)
    set_embedding_view(c, "set_embedding_view", v, n);
    CGE_CATCH(c)
}

// the fp64 entry points: a packed column-major host matrix, a packed device matrix of either layout
int cge_set_embedding(cge_ctx *c, const double *X, int64_t n, int64_t d) {
    if (!c || !X || n <= 0 || d <= 0) return CGE_E_ARG;
    const cge_embedding_view v = {X, d, 0, CGE_DTYPE_F64, 0, 0};
    CGE_TRY(c)
    set_embedding_view(c, "set_embedding", &v, n);
    CGE_CATCH(c)
}

int cge_set_embedding_device(cge_ctx *c, const double *X_dev, int64_t n, int64_t d, int row_major) {
    if (!c || !X_dev || n <= 0 || d <= 0) return CGE_E_ARG;
    const cge_embedding_view v = {X_dev, d, 0, CGE_DTYPE_F64, 1, row_major};
    CGE_TRY(c)
    set_embedding_view(c, "set_embedding_device", &v, n);
    CGE_CATCH(c)
}

} // extern "C"
