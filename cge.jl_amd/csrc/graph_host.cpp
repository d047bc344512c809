// graph_host.cpp -- the resident graph and vertex data: what cge_set_graph / cge_set_vertex_data do, as functions that throw
// (the C entries in capi.cpp and the internal callers -- cge_wgcl's init_* graph, exact mode -- call the same code), and the check
// that a landmark / score run makes of everything resident.
#include "common.hpp"

void set_graph(cge_ctx *c, const int64_t *src, const int64_t *dst, const double *w, i64 m, i64 n) {
    if (!src || !dst || m <= 0 || n <= 0 || n >= (1LL << 31)) throw CgeError{CGE_E_ARG, c->err}; // (a bare status: the message stays)
    // N > 1, option "shard_ingest": this rank uploads and keeps rows [e0, e1) of the list only (the edge passes are sums over
    // edges: every rank scatters what it holds and the all-reduce adds; the sampler's look-ups are exchanged, kernels_fit.hip).
    // Not for graphs small enough for the sampler to enumerate their non-edges on the host (wgcl_host.cpp).
    const bool shard = ingest_sharded(c) && (double)n * (double)(n - 1) > 33554432.0 && m >= c->coll.world;
    const i64 e0 = shard ? m * c->coll.rank / c->coll.world : 0, e1 = shard ? m * (c->coll.rank + 1) / c->coll.world : m;
    const i64 ml = e1 - e0;
    c->src.alloc_exact(ml);
    c->dst.alloc_exact(ml);
    // ids: validated and narrowed to 0-based int32 by the host workers on their way into the staging buffers
    std::atomic<i64> bad{-1};
    for (int col = 0; col < 2; col++) {
        const int64_t *h = (col ? dst : src) + e0;
        staged_upload<i32>(c, col ? c->dst.p : c->src.p, (size_t)ml, [&](i32 *o, size_t a0, size_t a1) {
            for (size_t e = a0; e < a1; e++) {
                const int64_t v = h[e];
                if (v < 1 || v > n) { i64 exp = -1; bad.compare_exchange_strong(exp, (i64)e); }
                o[e - a0] = (i32)(v - 1);
            }
        });
    }
    // (sharded: every rank must take the same exit -- the verdicts are exchanged before anybody throws)
    const bool any_bad = shard ? cge_allreduce_scalar_max(c, bad.load() >= 0 ? 1.0 : 0.0) != 0.0 : bad.load() >= 0;
    if (any_bad) {
        c->src.release(); c->dst.release(); c->m = c->m_total = 0; // (the previous resident graph is gone: cge_hip.h says so)
        c->blocked_ready = false; c->be_nchunks = 0; c->lm_ready = false;
        if (bad.load() >= 0)
            CGE_THROW(CGE_E_ARG, "edge %lld has a vertex id outside 1..%lld", (long long)(e0 + bad.load()) + 1, (long long)n);
        CGE_THROW(CGE_E_ARG, "an edge held by another rank has a vertex id outside 1..%lld", (long long)n);
    }
    // weights: all ones (an unweighted list, src/auxilary.jl:105) => neither a device copy nor a host mirror is kept
    bool unit = true;
    if (w) {
        const int nt = std::max(1, c->n_threads);
        std::vector<char> nonunit(nt, 0);
        const i64 per = (ml + nt - 1) / nt;
        const std::function<void(i64)> job = [&](i64 t) {
            const i64 a = std::min<i64>(ml, t * per), e = std::min<i64>(ml, a + per);
            char f = 0;
            for (i64 k = a; k < e && !f; k++) f = w[e0 + k] != 1.0;
            nonunit[t] = f;
        };
        c->pool->run(nt, job);
        for (char f : nonunit) unit = unit && !f;
    }
    if (shard) unit = cge_allreduce_scalar_max(c, unit ? 0.0 : 1.0) == 0.0;
    c->unit_weights = unit;
    c->h_w.clear();
    c->w.release();
    if (!unit) {
        c->h_w.assign(w + e0, w + e1); // mirror: weights of host-side sample draws
        c->w.alloc_exact(ml);
        staged_upload<double>(c, c->w.p, (size_t)ml, [&](double *o, size_t a0, size_t a1) { memcpy(o, w + e0 + a0, sizeof(double) * (a1 - a0)); });
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

void set_vertex_data(cge_ctx *c, const int64_t *comm, const double *vw, i64 n) {
    if (n <= 0) throw CgeError{CGE_E_ARG, c->err}; // (a bare status: the message stays)
    if (c->n && c->n != n) CGE_THROW(CGE_E_ASSERT, "No. communities (%lld) differ from no. nodes (%lld)", (long long)n, (long long)c->n);
    c->n = n;
    if (comm && c->rows_sharded) {
        // the rows are sharded BY COMMUNITY: another community vector is another ownership -- the resident rows are dropped
        // (upload the embedding again after this call)
        bool same = (i64)c->h_comm.size() == n;
        for (i64 i = 0; same && i < n; i++) same = c->h_comm[i] == (i32)(comm[i] - 1);
        if (!same) {
            c->Xr.release(); c->h_Xr.clear();
            c->d = 0;
            rows_unshard(c);
        }
    }
    if (comm) {
        c->h_comm.resize(n);
        i64 cmax = 0;
        for (i64 i = 0; i < n; i++) {
            if (comm[i] < 1) CGE_THROW(CGE_E_ARG, "community ids must be 1-based");
            c->h_comm[i] = (i32)(comm[i] - 1);
            cmax = std::max<i64>(cmax, comm[i]);
        }
        c->n_comm_max = cmax;
        c->comm.alloc_exact(n);
        HIP_CHECK(hipMemcpyAsync(c->comm.p, c->h_comm.data(), sizeof(i32) * n, hipMemcpyHostToDevice, c->stream));
        c->comm16.release();
        if (cmax < 65536) {
            const i64 npad = (n + CGE_COMM16_PAD - 1) / CGE_COMM16_PAD * CGE_COMM16_PAD; // whole vertex blocks (edge pass)
            std::vector<unsigned short> c16(npad, 0);
            for (i64 i = 0; i < n; i++) c16[i] = (unsigned short)c->h_comm[i];
            c->comm16.alloc_exact(npad);
            HIP_CHECK(hipMemcpyAsync(c->comm16.p, c16.data(), sizeof(unsigned short) * npad, hipMemcpyHostToDevice, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream)); // c16 goes out of scope
        }
    }
    if (vw) {
        c->h_vw.assign(vw, vw + n);
        c->vw.alloc_exact(n);
        HIP_CHECK(hipMemcpyAsync(c->vw.p, c->h_vw.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
    rows_refresh_local_tables(c);
    c->lm_ready = false;
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
