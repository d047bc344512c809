// graph_host.cpp -- the resident graph and vertex data: what cge_set_graph / cge_set_vertex_data do, as functions that throw
// (the C entries in capi.cpp and the internal callers -- cge_wgcl's init_* graph, exact mode -- call the same code), and the check
// that a landmark / score run makes of everything resident.
#include "common.hpp"

// ---- the boundary checks of a graph view (no context, no GPU) ---------------------------------------------------------------------
static size_t id_size(int id_dtype) { return id_dtype == CGE_ID_I64 ? 8 : 4; }
int graph_view_check(const cge_graph_view *g, i64 m, std::string &msg) {
    char b[256];
    b[0] = 0;
    if (!g) snprintf(b, sizeof b, "graph view: NULL view");
    else if (!g->src || !g->dst) snprintf(b, sizeof b, "graph view: NULL %s", g->src ? "dst" : "src");
    else if (m <= 0) snprintf(b, sizeof b, "graph view: m = %lld (must be positive)", (long long)m);
    else if (g->stride < 1) snprintf(b, sizeof b, "graph view: stride %lld (must be >= 1)", (long long)g->stride);
    else if (g->id_dtype != CGE_ID_I64 && g->id_dtype != CGE_ID_I32) snprintf(b, sizeof b, "graph view: unknown id dtype %d", g->id_dtype);
    else if (g->base < -1 || g->base > 1) snprintf(b, sizeof b, "graph view: base %d (0, 1, or -1 to infer it)", g->base);
    else if (g->w && g->w_dtype != CGE_DTYPE_F64 && g->w_dtype != CGE_DTYPE_F32)
        snprintf(b, sizeof b, "graph view: weights of dtype %d (fp64 or fp32: widening fp16 / bf16 weights is left to the caller)", g->w_dtype);
    else if ((uintptr_t)g->src % id_size(g->id_dtype) != 0 || (uintptr_t)g->dst % id_size(g->id_dtype) != 0)
        snprintf(b, sizeof b, "graph view: src / dst not aligned to their %d-byte ids", (int)id_size(g->id_dtype));
    else if (g->w && (uintptr_t)g->w % (g->w_dtype == CGE_DTYPE_F64 ? 8 : 4) != 0) snprintf(b, sizeof b, "graph view: weights not aligned to their elements");
    else {
        // the two columns may share memory only as the interleaved columns their stride describes: dst = src +- k elements, 0 < k < stride
        const i64 es = (i64)id_size(g->id_dtype);
        const double span = ((double)(m - 1) * (double)g->stride + 1.0) * (double)es; // bytes a column reaches over
        const intptr_t diff = (intptr_t)((uintptr_t)g->dst - (uintptr_t)g->src);
        const double dist = diff < 0 ? -(double)diff : (double)diff;
        if (dist < span && !(diff != 0 && dist < (double)g->stride * (double)es))
            snprintf(b, sizeof b, "graph view: src and dst overlap (%lld bytes apart) in a way stride %lld does not explain", (long long)diff,
                     (long long)g->stride);
        else return CGE_OK;
    }
    msg = b;
    return CGE_E_ARG;
}

// ---- the graph ingest -------------------------------------------------------------------------------------------------------------
static void drop_graph(cge_ctx *c) { // (the previous resident graph is gone: cge_hip.h says so)
    c->src.release(); c->dst.release(); c->m = c->m_total = 0;
    c->blocked_ready = false; c->be_nchunks = 0; c->lm_ready = false;
}
static void atomic_min(std::atomic<i64> &a, i64 v) {
    i64 cur = a.load();
    while (v < cur && !a.compare_exchange_weak(cur, v)) {}
}
// minimum and maximum id of both columns of a host view (all m edges: every rank of a sharded upload decides alike)
template <class I>
static void host_extrema(cge_ctx *c, const cge_graph_view *g, i64 m, i64 &lo, i64 &hi) {
    const I *s = (const I *)g->src, *d = (const I *)g->dst;
    const i64 st = g->stride;
    const int nt = std::max(1, c->n_threads);
    std::vector<i64> los(nt, INT64_MAX), his(nt, INT64_MIN);
    const i64 per = (m + nt - 1) / nt;
    const std::function<void(i64)> job = [&](i64 t) {
        const i64 a = std::min<i64>(m, t * per), e = std::min<i64>(m, a + per);
        i64 l = INT64_MAX, h = INT64_MIN;
        for (i64 k = a; k < e; k++) {
            const i64 u = (i64)s[k * st], v = (i64)d[k * st];
            l = std::min(l, std::min(u, v));
            h = std::max(h, std::max(u, v));
        }
        los[t] = l; his[t] = h;
    };
    c->pool->run(nt, job);
    lo = *std::min_element(los.begin(), los.end());
    hi = *std::max_element(his.begin(), his.end());
}
// ids of edges [e0, e0 + ml) of a host column: checked on the 64-bit value, narrowed to 0-based int32 by the host workers on their
// way into the staging buffers.  STRIDE 1 / 2: the two common layouts with a constant step; 0: any stride.
template <class I, int STRIDE>
static void upload_ids(cge_ctx *c, const I *h, i64 stride, i64 base, i64 n, i64 e0, i64 ml, i32 *dev, std::atomic<i64> &bad) {
    const i64 st = STRIDE ? STRIDE : stride;
    staged_upload<i32>(c, dev, (size_t)ml, [&](i32 *o, size_t a0, size_t a1) {
        const I *p = h + (e0 + (i64)a0) * st;
        i64 first = -1;
        for (size_t e = a0; e < a1; e++, p += st) {
            const uint64_t v = (uint64_t)(i64)*p - (uint64_t)base; // (an id below the base wraps beyond every n)
            if (v >= (uint64_t)n && first < 0) first = (i64)e;
            o[e - a0] = (i32)v;
        }
        if (first >= 0) atomic_min(bad, first);
    });
}
template <class I>
static void upload_ids_any(cge_ctx *c, const void *h, i64 stride, i64 base, i64 n, i64 e0, i64 ml, i32 *dev, std::atomic<i64> &bad) {
    if (stride == 1) upload_ids<I, 1>(c, (const I *)h, stride, base, n, e0, ml, dev, bad);
    else if (stride == 2) upload_ids<I, 2>(c, (const I *)h, stride, base, n, e0, ml, dev, bad);
    else upload_ids<I, 0>(c, (const I *)h, stride, base, n, e0, ml, dev, bad);
}
// the base (given, or the minimum id: 0 or 1 as parseargs demands, src/auxilary.jl:92-98) and the vertex count (given, or the
// maximum id, :99) from the extrema
static void settle_base_and_n(cge_ctx *c, i64 lo, i64 hi, i64 &base, i64 &n) {
    if (base < 0) {
        if (lo != 0 && lo != 1) { drop_graph(c); CGE_THROW(CGE_E_ASSERT, "Vertices should be either 0-based or 1-based"); }
        base = lo;
    }
    if (n == 0) {
        const i64 top = hi >= base ? hi - base + 1 : 0; // (an overflow of hi - base + 1 needs hi near 2^63: refused below as too many)
        if (hi < base || hi - base >= (1LL << 31) - 1) {
            drop_graph(c);
            CGE_THROW(CGE_E_ARG, "the maximum vertex id %lld gives no vertex count below 2^31 (base %lld)", (long long)hi, (long long)base);
        }
        n = top;
    }
}

void set_graph_view(cge_ctx *c, const char *who, const cge_graph_view *g, i64 m, i64 n) {
    std::string msg;
    if (graph_view_check(g, m, msg) != CGE_OK) CGE_THROW(CGE_E_ARG, "%s: %s", who, msg.c_str());
    if (n < 0 || n >= (1LL << 31)) CGE_THROW(CGE_E_ARG, "%s: n = %lld (0 .. 2^31 - 1; 0 = the maximum id)", who, (long long)n);
    link_drop(c); // (a link model refers to the resident graph)
    const bool dev = g->on_device != 0, i64ids = g->id_dtype == CGE_ID_I64;
    if (dev) {
        check_device_pointer(c, who, g->src);
        check_device_pointer(c, who, g->dst);
        if (g->w) check_device_pointer(c, who, g->w);
    }
    i64 base = g->base;
    DevBuf<i64> scal; // two words of the device passes: the extrema, then the lowest bad edge and the weights' verdict
    if (base < 0 || n == 0) {
        i64 mm[2] = {0, 0};
        if (dev) {
            scal.alloc_exact(2);
            k_id_extrema(c, g->src, g->dst, g->stride, g->id_dtype, m, scal.p);
            HIP_CHECK(hipMemcpyAsync(mm, scal.p, sizeof mm, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        } else if (i64ids) host_extrema<int64_t>(c, g, m, mm[0], mm[1]);
        else host_extrema<int32_t>(c, g, m, mm[0], mm[1]);
        settle_base_and_n(c, mm[0], mm[1], base, n);
    }
    // N > 1, option "shard_ingest": this rank uploads and keeps rows [e0, e1) of the list only (the edge passes are sums over
    // edges: every rank scatters what it holds and the all-reduce adds; the sampler's look-ups are exchanged, kernels_fit.hip).
    // Not for graphs small enough for the sampler to enumerate their non-edges on the host (wgcl_host.cpp), nor for a device view.
    const bool shard = !dev && ingest_sharded(c) && (double)n * (double)(n - 1) > 33554432.0 && m >= c->coll.world;
    const i64 e0 = shard ? m * c->coll.rank / c->coll.world : 0, e1 = shard ? m * (c->coll.rank + 1) / c->coll.world : m;
    const i64 ml = e1 - e0;
    c->src.alloc_exact(ml);
    c->dst.alloc_exact(ml);
    std::atomic<i64> bad{INT64_MAX}; // the lowest edge (of this rank's) with an id outside the vertex range
    bool unit = true;
    DevBuf<double> wdev;
    if (dev) {
        if (!scal.p) scal.alloc_exact(2);
        if (g->w) wdev.alloc_exact(ml);
        k_graph_ingest(c, g->src, g->dst, g->stride, g->id_dtype, base, n, g->w, g->w_dtype, m, c->src.p, c->dst.p, wdev.p, scal.p);
        i64 fl[2] = {m, 0};
        HIP_CHECK(hipMemcpyAsync(fl, scal.p, sizeof fl, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream)); // (the caller may free or reuse its buffers on return)
        if (fl[0] < m) bad.store(fl[0]);
        unit = fl[1] == 0;
    } else {
        // ids: validated and narrowed to 0-based int32 by the host workers on their way into the staging buffers
        for (int col = 0; col < 2; col++) {
            const void *h = col ? g->dst : g->src;
            if (i64ids) upload_ids_any<int64_t>(c, h, g->stride, base, n, e0, ml, col ? c->dst.p : c->src.p, bad);
            else upload_ids_any<int32_t>(c, h, g->stride, base, n, e0, ml, col ? c->dst.p : c->src.p, bad);
        }
    }
    // (sharded: every rank must take the same exit -- the verdicts are exchanged before anybody throws)
    const bool mine = bad.load() != INT64_MAX;
    const bool any_bad = shard ? cge_allreduce_scalar_max(c, mine ? 1.0 : 0.0) != 0.0 : mine;
    if (any_bad) {
        drop_graph(c);
        if (mine)
            CGE_THROW(CGE_E_ARG, "edge %lld has a vertex id outside %lld..%lld", (long long)(e0 + bad.load()) + 1, (long long)base, (long long)(base + n - 1));
        CGE_THROW(CGE_E_ARG, "an edge held by another rank has a vertex id outside %lld..%lld", (long long)base, (long long)(base + n - 1));
    }
    // weights: all ones (an unweighted list, src/auxilary.jl:105) => neither a device copy nor a host mirror is kept
    const bool f32 = g->w_dtype == CGE_DTYPE_F32;
    const double *w64 = (const double *)g->w;
    const float *w32 = (const float *)g->w;
    if (g->w && !dev) {
        const int nt = std::max(1, c->n_threads);
        std::vector<char> nonunit(nt, 0);
        const i64 per = (ml + nt - 1) / nt;
        const std::function<void(i64)> job = [&](i64 t) {
            const i64 a = std::min<i64>(ml, t * per), e = std::min<i64>(ml, a + per);
            char f = 0;
            if (f32) for (i64 k = a; k < e && !f; k++) f = w32[e0 + k] != 1.0f;
            else for (i64 k = a; k < e && !f; k++) f = w64[e0 + k] != 1.0;
            nonunit[t] = f;
        };
        c->pool->run(nt, job);
        for (char f : nonunit) unit = unit && !f;
    }
    if (shard) unit = cge_allreduce_scalar_max(c, unit ? 0.0 : 1.0) == 0.0;
    c->unit_weights = unit;
    c->h_w.clear();
    c->w.release();
    if (!unit) { // the device copy and its host mirror (weights of host-side sample draws)
        if (dev) {
            c->w.swap(wdev);
            c->h_w.resize(ml);
            HIP_CHECK(hipMemcpyAsync(c->h_w.data(), c->w.p, sizeof(double) * ml, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        } else {
            if (f32) c->h_w.assign(w32 + e0, w32 + e1); // (widening is exact)
            else c->h_w.assign(w64 + e0, w64 + e1);
            c->w.alloc_exact(ml);
            const double *hw = c->h_w.data();
            staged_upload<double>(c, c->w.p, (size_t)ml, [=](double *o, size_t a0, size_t a1) { memcpy(o, hw + a0, sizeof(double) * (a1 - a0)); });
        }
    }
    c->m_total = m;
    c->e_first = e0;
    c->edges_sharded = shard;
    c->m = ml;
    if (c->n && c->n != n) { // another vertex set: nothing that was sized for the old one may survive (stale or short buffers)
        c->h_Xr.clear(); c->h_vw.clear(); c->h_comm.clear();
        c->Xr.release(); c->Xc.release(); c->rnorm.release(); c->vw.release(); c->comm.release(); c->comm16.release();
        c->d = 0;
        c->centred_ready = false;
        rows_unshard(c);
    }
    c->n = n;
    c->lm_ready = false;
    c->blocked_ready = false; // the blocked copy of the edge list is rebuilt by the first edge pass
}

// cge_set_graph: the view of two 1-based int64 host columns with fp64 weights
void set_graph(cge_ctx *c, const int64_t *src, const int64_t *dst, const double *w, i64 m, i64 n) {
    if (!src || !dst || m <= 0 || n <= 0 || n >= (1LL << 31)) throw CgeError{CGE_E_ARG, c->err}; // (a bare status: the message stays)
    const cge_graph_view g = {src, dst, 1, CGE_ID_I64, 1, w, CGE_DTYPE_F64, 0};
    set_graph_view(c, "set_graph", &g, m, n);
}

// ---- the vertex data ---------------------------------------------------------------------------------------------------------------
// extrema of n host ids
template <class I>
static void host_id_range(const void *ids, i64 n, i64 &lo, i64 &hi) {
    const I *p = (const I *)ids;
    lo = INT64_MAX; hi = INT64_MIN;
    for (i64 i = 0; i < n; i++) { lo = std::min<i64>(lo, (i64)p[i]); hi = std::max<i64>(hi, (i64)p[i]); }
}
static void derive_vertex_weights(cge_ctx *c, const char *who, i64 n) {
    if (!c->src.p || c->m <= 0 || c->n != n)
        CGE_THROW(CGE_E_ARG, "%s: vertex weights are derived from the resident edge list: upload the graph (of %lld vertices) first", who, (long long)n);
    if (c->edges_sharded)
        CGE_THROW(CGE_E_ARG, "%s: the resident edge list is sharded over the ranks (option shard_ingest): a sum in edge order cannot be "
                             "assembled from per-rank partial sums -- pass the vertex weights", who);
    c->vw.alloc_exact(n);
    if (c->unit_weights) k_vertex_weights_unit(c, c->src.p, c->dst.p, c->m, n, c->vw.p);
    else {
        if (c->m >= (1LL << 30)) CGE_THROW(CGE_E_ARG, "%s: derived vertex weights of a weighted list are limited to 2^30 edges", who);
        k_vertex_weights_ordered(c, c->src.p, c->dst.p, c->w.p, c->m, n, c->vw.p);
    }
    c->h_vw.resize(n);
    HIP_CHECK(hipMemcpyAsync(c->h_vw.data(), c->vw.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
}

void set_vertex_view(cge_ctx *c, const char *who, const cge_vertex_view *v, i64 n, bool derive_vw) {
    if (!v || n <= 0) throw CgeError{CGE_E_ARG, c->err}; // (a bare status: the message stays)
    link_drop(c); // (a link model refers to the resident vertex data)
    const bool dev = v->on_device != 0;
    if (v->comm) {
        if (v->id_dtype != CGE_ID_I64 && v->id_dtype != CGE_ID_I32) CGE_THROW(CGE_E_ARG, "%s: unknown id dtype %d", who, v->id_dtype);
        if (v->base < -1 || v->base > 1) CGE_THROW(CGE_E_ARG, "%s: base %d (0, 1, or -1 to infer it)", who, v->base);
        if ((uintptr_t)v->comm % id_size(v->id_dtype) != 0) CGE_THROW(CGE_E_ARG, "%s: comm not aligned to its %d-byte ids", who, (int)id_size(v->id_dtype));
        if (dev) check_device_pointer(c, who, v->comm);
    }
    if (v->vweights) {
        if (v->vw_dtype != CGE_DTYPE_F64 && v->vw_dtype != CGE_DTYPE_F32) CGE_THROW(CGE_E_ARG, "%s: vertex weights of dtype %d (fp64 or fp32)", who, v->vw_dtype);
        if ((uintptr_t)v->vweights % (v->vw_dtype == CGE_DTYPE_F64 ? 8 : 4) != 0) CGE_THROW(CGE_E_ARG, "%s: vertex weights not aligned to their elements", who);
        if (dev) check_device_pointer(c, who, v->vweights);
    }
    if (c->n && c->n != n) CGE_THROW(CGE_E_ASSERT, "No. communities (%lld) differ from no. nodes (%lld)", (long long)n, (long long)c->n);
    c->n = n;
    if (v->comm) {
        const bool i64ids = v->id_dtype == CGE_ID_I64;
        i64 lo = 0, hi = 0, base = v->base;
        DevBuf<i64> scal;
        if (dev) {
            i64 mm[2];
            scal.alloc_exact(2);
            k_id_extrema(c, v->comm, nullptr, 1, v->id_dtype, n, scal.p);
            HIP_CHECK(hipMemcpyAsync(mm, scal.p, sizeof mm, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
            lo = mm[0]; hi = mm[1];
        } else if (i64ids) host_id_range<int64_t>(v->comm, n, lo, hi);
        else host_id_range<int32_t>(v->comm, n, lo, hi);
        if (base < 0) { // src/auxilary.jl:133-134
            if (lo != 0 && lo != 1) CGE_THROW(CGE_E_ASSERT, "Communities should be either 0-based or 1-based, but are %lld based.", (long long)lo);
            base = lo;
        }
        if (lo < base) CGE_THROW(CGE_E_ARG, base == 1 ? "community ids must be 1-based" : "community ids must be 0-based");
        if (hi - base >= (1LL << 31) - 1) CGE_THROW(CGE_E_ARG, "%s: community id %lld does not fit the tables", who, (long long)hi);
        const i64 cmax = hi - base + 1;
        const i64 npad = (n + CGE_COMM16_PAD - 1) / CGE_COMM16_PAD * CGE_COMM16_PAD; // whole vertex blocks (edge pass)
        std::vector<i32> hc(n);
        DevBuf<i32> dcomm;
        DevBuf<unsigned short> dcomm16;
        if (dev) { // rebased and narrowed on the device; the host mirror is one copy back
            dcomm.alloc_exact(n);
            if (cmax < 65536) {
                dcomm16.alloc_exact(npad);
                HIP_CHECK(hipMemsetAsync(dcomm16.p, 0, sizeof(unsigned short) * npad, c->stream));
            }
            k_vertex_ingest(c, v->comm, v->id_dtype, base, n, dcomm.p, dcomm16.p);
            HIP_CHECK(hipMemcpyAsync(hc.data(), dcomm.p, sizeof(i32) * n, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        } else if (i64ids) for (i64 i = 0; i < n; i++) hc[i] = (i32)(((const int64_t *)v->comm)[i] - base);
        else for (i64 i = 0; i < n; i++) hc[i] = (i32)((i64)((const int32_t *)v->comm)[i] - base);
        if (c->rows_sharded && c->h_comm != hc) {
            // the rows are sharded BY COMMUNITY: another community vector is another ownership -- the resident rows are dropped
            // (upload the embedding again after this call)
            c->Xr.release(); c->h_Xr.clear();
            c->d = 0;
            rows_unshard(c);
        }
        c->h_comm.swap(hc);
        c->n_comm_max = cmax;
        c->comm16.release();
        if (dev) {
            c->comm.swap(dcomm);
            if (dcomm16.p) c->comm16.swap(dcomm16);
        } else {
            c->comm.alloc_exact(n);
            HIP_CHECK(hipMemcpyAsync(c->comm.p, c->h_comm.data(), sizeof(i32) * n, hipMemcpyHostToDevice, c->stream));
            if (cmax < 65536) {
                std::vector<unsigned short> c16(npad, 0);
                for (i64 i = 0; i < n; i++) c16[i] = (unsigned short)c->h_comm[i];
                c->comm16.alloc_exact(npad);
                HIP_CHECK(hipMemcpyAsync(c->comm16.p, c16.data(), sizeof(unsigned short) * npad, hipMemcpyHostToDevice, c->stream));
                HIP_CHECK(hipStreamSynchronize(c->stream)); // c16 goes out of scope
            }
        }
    }
    if (v->vweights) {
        const bool f32 = v->vw_dtype == CGE_DTYPE_F32;
        c->vw.alloc_exact(n);
        c->h_vw.resize(n);
        if (dev) { // widened on the device (exact); the host mirror is one copy back
            k_ingest_rows(c, v->vweights, v->vw_dtype, n, 1, n, c->vw.p);
            HIP_CHECK(hipMemcpyAsync(c->h_vw.data(), c->vw.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        } else {
            if (f32) for (i64 i = 0; i < n; i++) c->h_vw[i] = (double)((const float *)v->vweights)[i];
            else memcpy(c->h_vw.data(), v->vweights, sizeof(double) * n);
            HIP_CHECK(hipMemcpyAsync(c->vw.p, c->h_vw.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        }
    } else if (derive_vw)
        derive_vertex_weights(c, who, n);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    rows_refresh_local_tables(c);
    c->lm_ready = false;
}

// cge_set_vertex_data: the view of 1-based int64 host ids and fp64 weights; NULL weights leave the resident ones
void set_vertex_data(cge_ctx *c, const int64_t *comm, const double *vw, i64 n) {
    const cge_vertex_view v = {comm, CGE_ID_I64, 1, vw, CGE_DTYPE_F64, 0};
    set_vertex_view(c, "set_vertex_data", &v, n, false);
}

// clusters::Vector{Vector{Int}} as parseargs builds it from comm (src/auxilary.jl:199-208): one cluster per community that occurs,
// its members in ascending vertex id -- a counting sort of the host mirror.  (The reference collects the values of a Dict, in no
// particular order; runsplit sorts the clusters itself.)
void clusters_from_comm(const cge_ctx *c, std::vector<i64> &flat, std::vector<i64> &off) {
    const i64 n = c->n, C = c->n_comm_max;
    if (n <= 0 || (i64)c->h_comm.size() != n || C <= 0)
        CGE_THROW(CGE_E_ARG, "clusters from communities (n_clusters = -1): no communities are resident (cge_set_vertex_data / cge_set_vertex_view)");
    std::vector<i64> at(C + 1, 0);
    for (i64 i = 0; i < n; i++) at[c->h_comm[i] + 1]++;
    off.assign(1, 0);
    for (i64 q = 0; q < C; q++) {
        const i64 cnt = at[q + 1];
        at[q + 1] = at[q] + cnt; // at[q]: where community q's members start
        if (cnt > 0) off.push_back(off.back() + cnt);
    }
    flat.resize(n);
    std::vector<i64> next(at.begin(), at.end() - 1);
    for (i64 i = 0; i < n; i++) flat[next[c->h_comm[i]]++] = i + 1;
}

// the resident inputs a landmark / score run reads: all present and all sized for the same vertex set
void check_resident(cge_ctx *c, const char *who) {
    if (!c->Xr.p || !c->vw.p || !c->comm.p || !c->src.p)
        CGE_THROW(CGE_E_ARG, "%s: graph, embedding and vertex data must be resident (cge_set_graph / cge_set_embedding / "
                             "cge_set_vertex_data; a cge_wgcl call in exact mode replaces the resident graph)", who);
    const size_t n = (size_t)c->n;
    const size_t rows = (size_t)lm_rows(c);
    if (c->rows_sharded && (!c->vw_loc.p || !c->comm_loc.p))
        CGE_THROW(CGE_E_ARG, "%s: option shard_rows needs the vertex weights and communities resident (cge_set_vertex_data)", who);
    if (c->n <= 0 || c->d <= 0 || c->m <= 0 || c->Xr.n < rows * (size_t)c->d || c->vw.n < n || c->comm.n < n ||
        c->src.n < (size_t)c->m || c->dst.n < (size_t)c->m)
        CGE_THROW(CGE_E_ARG, "%s: resident inputs are inconsistent (n = %lld, d = %lld, m = %lld): upload them again", who,
                  (long long)c->n, (long long)c->d, (long long)c->m);
}
