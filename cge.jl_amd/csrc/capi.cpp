// capi.cpp -- the extern "C" surface declared in include/cge_hip.h: argument checks, the context's device, a call into a host
// module (graph_host / embedding_host / landmarks_host / diameter_host / score_host / batch_host; collectives.cpp has the
// entries of the rank exchange), scalars copied out, an exception turned into a status.  Also the option and statistics tables,
// the profiling entries and the test hooks of include/cge_hip_testing.h.
#include "common.hpp"
#include "../../include/cge_hip_testing.h"

// the event pairs of the finished launches become milliseconds; the events go back to the pool
void flush_timers(cge_ctx *c) {
    for (auto &kv : c->timers) {
        for (auto &pr : kv.second.pending) {
            float ms = 0.f;
            (void)hipEventSynchronize(pr.second);
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) kv.second.total_ms += ms;
            c->event_pool.push_back(pr.first);
            c->event_pool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}
template <class Map> // the keys of a map, comma-separated, into the caller's buffer
static int key_names(const Map &m, char *buf, int64_t buf_len) {
    std::string s;
    for (auto &kv : m) s += (s.empty() ? "" : ",") + kv.first;
    snprintf(buf, (size_t)buf_len, "%s", s.c_str());
    return CGE_OK;
}

extern "C" {

int cge_abi_version(void) { return CGE_ABI_VERSION; }

int cge_create(cge_ctx **out, int device, void *stream) {
    if (!out) return CGE_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CGE_E_HIP; // no GPU: fail loudly, no fallback
    if (device < 0 || device >= ndev) return CGE_E_ARG;
    cge_ctx *c = new (std::nothrow) cge_ctx();
    if (!c) return CGE_E_OOM;
    try {
        HIP_CHECK(hipSetDevice(device));
        c->device = device;
        if (stream) {
            c->stream = (hipStream_t)stream;
        } else {
            HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
            c->own_stream = true;
        }
        HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&c->copy_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming));
        for (hipEvent_t *ev : {c->sweep_ev, c->tab_ev, c->stage_ev})
            for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        unsigned hc = std::thread::hardware_concurrency();
        c->n_threads = (int)std::max(1u, std::min(hc ? hc : 8u, 16u));
        c->pool = new ThreadPool(c->n_threads - 1);
        // the pinned staging buffers of the uploads: made here, once per context, not inside the first cge_set_graph (pinning
        // 128 MiB is ~10 ms of page work that has nothing to do with any graph)
        for (int b = 0; b < 2; b++) c->stage[b].ensure(CGE_STAGE_BYTES);
        { // ... and the copy path itself walked once (the first host-to-device copy of a process sets up the DMA queues)
            DevBuf<unsigned char> warm;
            warm.ensure((size_t)1 << 20);
            for (int b = 0; b < 2; b++) {
                memset(c->stage[b].p, 0, (size_t)1 << 20);
                HIP_CHECK(hipMemcpyAsync(warm.p, c->stage[b].p, (size_t)1 << 20, hipMemcpyHostToDevice, c->stream));
            }
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        if (const char *nap = getenv("CGE_FIT_TEST_DELAY")) { // stress runs of whole suites: option fit_persistent_test_delay for
            // every context.  A testing knob in a production path: clamped to 2000 naps (~6 ms, far below the 1 s hand-off
            // deadline, so it can never force the time-out path) and announced once per process.
            c->opt_fit_test_delay = std::max(0, std::min(atoi(nap), 2000));
            static std::atomic<bool> told{false};
            if (c->opt_fit_test_delay > 0 && !told.exchange(true))
                fprintf(stderr, "cge: CGE_FIT_TEST_DELAY=%d is set: every persistent fit starts its tile waves late (testing knob)\n",
                        c->opt_fit_test_delay);
        }
    } catch (const CgeError &e) {
        delete c;
        return e.code;
    }
    *out = c;
    return CGE_OK;
}

void cge_destroy(cge_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    flush_timers(c);
    (void)cge_comm_finalize(c);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    c->event_pool.clear();
    if (c->copy_ev) (void)hipEventDestroy(c->copy_ev);
    if (c->copy_done) (void)hipEventDestroy(c->copy_done);
    if (c->samp_ev) (void)hipEventDestroy(c->samp_ev);
    for (hipEvent_t *ev : {c->sweep_ev, c->tab_ev, c->stage_ev})
        for (int i = 0; i < 2; i++)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    delete c->pool;
    c->pool = nullptr;
    delete c;
}

const char *cge_last_error(const cge_ctx *c) { return c ? c->err.c_str() : "null context"; }

int cge_set_host_threads(cge_ctx *c, int n) {
    if (!c || n < 1) return CGE_E_ARG;
    c->n_threads = n;
    delete c->pool;
    c->pool = new ThreadPool(n - 1);
    return CGE_OK;
}

// ---- resident inputs ------------------------------------------------------------------------------
int cge_set_graph(cge_ctx *c, const int64_t *src, const int64_t *dst, const double *w, int64_t m, int64_t n) {
    if (!c) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    set_graph(c, src, dst, w, m, n);
    CGE_CATCH(c)
}

int cge_set_vertex_data(cge_ctx *c, const int64_t *comm, const double *vw, int64_t n) {
    if (!c) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    set_vertex_data(c, comm, vw, n);
    CGE_CATCH(c)
}

// the graph and vertex views (graph_host.cpp): cge_set_graph / cge_set_vertex_data above are shorthands for them
int cge_graph_view_check(const cge_graph_view *g, int64_t m, char *err, int64_t err_len) {
    std::string msg;
    const int rc = graph_view_check(g, m, msg);
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", msg.c_str());
    return rc;
}
int cge_set_graph_view(cge_ctx *c, const cge_graph_view *g, int64_t m, int64_t n, int64_t *n_out) {
    if (!c || !g) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    set_graph_view(c, "set_graph_view", g, m, n);
    if (n_out) *n_out = c->n;
    CGE_CATCH(c)
}
int cge_set_vertex_view(cge_ctx *c, const cge_vertex_view *v, int64_t n) {
    if (!c || !v) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    set_vertex_view(c, "set_vertex_view", v, n, true);
    CGE_CATCH(c)
}
int cge_vertex_weights(cge_ctx *c, double *out, int64_t n) {
    if (!c || !out) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (!c->vw.p || n != c->n || (i64)c->h_vw.size() != n) CGE_THROW(CGE_E_ARG, "vertex_weights: no vertex weights of %lld vertices are resident", (long long)n);
    memcpy(out, c->h_vw.data(), sizeof(double) * (size_t)n);
    CGE_CATCH(c)
}

// ---- landmarks ------------------------------------------------------------------------------------
int cge_landmarks_run(cge_ctx *c, const int64_t *cl_flat, const int64_t *cl_off, int64_t ncl, int64_t land,
                      int64_t forced, int method, int directed, int64_t *N_out, int64_t *n_ledges_out, int *truncated) {
    if (!c || (ncl != -1 && (!cl_flat || !cl_off))) return CGE_E_ARG; // (n_clusters = -1: derived from the resident communities)
    CGE_TRY_ON_DEVICE(c)
    host_landmarks_run(c, LandmarkRun{cl_flat, cl_off, ncl, land, forced, method, directed, true});
    if (N_out) *N_out = c->N;
    if (n_ledges_out) *n_ledges_out = c->n_ledges;
    if (truncated) *truncated = c->lm_truncated;
    CGE_CATCH(c)
}

int cge_landmarks_info(cge_ctx *c, int64_t *N_out, int64_t *n_ledges_out, int *truncated) {
    if (!c) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_landmarks_info(c);
    if (N_out) *N_out = c->N;
    if (n_ledges_out) *n_ledges_out = c->n_ledges;
    if (truncated) *truncated = c->lm_truncated;
    CGE_CATCH(c)
}

int cge_landmarks_fetch(cge_ctx *c, double *dii, double *embed, int64_t *cluster, int64_t *ledges, double *lw_e,
                        double *lweight, int64_t *v_to_l) {
    if (!c) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_landmarks_fetch(c, dii, embed, cluster, ledges, lw_e, lweight, v_to_l);
    CGE_CATCH(c)
}

int cge_runsplit(cge_ctx *c, const int64_t *cl_flat, const int64_t *cl_off, int64_t ncl, int64_t nland,
                 int64_t forced, int method, int64_t *group_ids) {
    if (!c || !group_ids) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (!c->Xr.p || !c->vw.p) CGE_THROW(CGE_E_ARG, "runsplit: embedding and vertex weights must be resident");
    std::vector<i64> gid;
    host_runsplit(c, cl_flat, cl_off, ncl, nland, forced, method, gid);
    memcpy(group_ids, gid.data(), sizeof(i64) * c->n);
    CGE_CATCH(c)
}

// ---- samples --------------------------------------------------------------------------------------
int cge_draw_samples(cge_ctx *c, int64_t seed, int64_t stream_id, int64_t S, int directed, int64_t *pos_idx,
                     int64_t *neg_i, int64_t *neg_j) {
    if (!c || S <= 0 || !pos_idx || !neg_i || !neg_j) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (!c->src.p) CGE_THROW(CGE_E_ARG, "draw_samples: no resident graph");
    if (c->edges_sharded) CGE_THROW(CGE_E_ARG, "draw_samples: the resident edge list is sharded over the ranks (option shard_ingest); cge_score draws on the device");
    host_draw_samples(c, seed, stream_id, S, directed, pos_idx, neg_i, neg_j);
    CGE_CATCH(c)
}

int cge_max_pair_dist(cge_ctx *c, int part, int nparts, double *hi, int64_t *arg_i, int64_t *arg_j) {
    if (!c || !hi || nparts < 1 || part < 0 || part >= nparts) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    *hi = host_diameter_brute(c, part, nparts, arg_i, arg_j);
    CGE_CATCH(c)
}

// ---- wGCL -------------------------------------------------------------------------------------------
int cge_wgcl(cge_ctx *c, const cge_wgcl_args *a, double out[7], int *out_len, cge_trace *trace) {
    if (!c || !a || !out || !out_len) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_wgcl(c, a, out, out_len, trace);
    CGE_CATCH(c)
}

int cge_score(cge_ctx *c, const cge_score_args *a, double out[7], int *out_len, cge_trace *trace) {
    if (!c || !a || !out || !out_len) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_score(c, a, out, out_len, trace, nullptr, false);
    CGE_CATCH(c)
}

// cge_score_batch: K embeddings of the resident graph (batch_host.cpp); a member is a cge_embedding_view
int cge_score_batch(cge_ctx *c, const cge_score_args *a, const cge_embedding_batch *b, double *out, int *out_len,
                    cge_trace *traces) {
    if (!c || !a || !b || !out || !out_len || !b->embeddings || b->K < 1 || b->d <= 0 || (b->row_major && !b->on_device))
        return CGE_E_ARG;
    std::vector<cge_embedding_view> views; // K packed fp64 views of one shape (a NULL member: the view check refuses it)
    try {
        for (i64 k = 0; k < b->K; k++) views.push_back({b->embeddings[k], b->d, 0, CGE_DTYPE_F64, b->on_device, b->row_major});
    } catch (const std::bad_alloc &) {
        return CGE_E_OOM;
    }
    return score_batch_run(c, a, views.data(), b->K, "score_batch", out, out_len, traces);
}
int cge_score_views(cge_ctx *c, const cge_score_args *a, const cge_embedding_view *views, int64_t K, double *out, int *out_len,
                    cge_trace *traces) {
    if (!c || !a || !views || !out || !out_len || K < 1) return CGE_E_ARG;
    return score_batch_run(c, a, views, K, "score_views", out, out_len, traces);
}

// ---- link prediction under the fitted model (link_host.cpp) -------------------------------------------
int cge_link_fit(cge_ctx *c, const cge_score_args *a, int which, double out[7], int *out_len, cge_trace *trace) {
    if (!c || !a || !out || !out_len) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_fit(c, a, which, out, out_len, trace);
    CGE_CATCH(c)
}
int cge_link_set_model(cge_ctx *c, int directed, double alpha, double hi, const double *f_out, const double *f_in, int64_t n) {
    if (!c || !f_out) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_set_model(c, directed, alpha, hi, f_out, f_in, n);
    CGE_CATCH(c)
}
int cge_link_model_fetch(cge_ctx *c, int *directed, double *alpha, double *hi, double *f_out, double *f_in, double *T_out,
                         double *T_in, int64_t *N) {
    if (!c) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_model_fetch(c, directed, alpha, hi, f_out, f_in, T_out, T_in, N);
    CGE_CATCH(c)
}
int cge_link_prob(cge_ctx *c, const int64_t *i, const int64_t *j, int64_t P, double *out) {
    if (!c || !i || !j || !out) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_prob(c, i, j, P, out);
    CGE_CATCH(c)
}
int cge_link_topk(cge_ctx *c, const int64_t *queries, int64_t Q, int64_t k, int exclude_edges, int64_t *out_j, double *out_p,
                  int64_t *out_cnt) {
    if (!c || !queries || !out_j || !out_p || !out_cnt) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_topk(c, queries, Q, k, exclude_edges, out_j, out_p, out_cnt);
    CGE_CATCH(c)
}
int cge_link_rank(cge_ctx *c, const int64_t *i, const int64_t *j, int64_t P, int exclude_edges, int64_t *out_greater,
                  int64_t *out_ties, int64_t *out_cand, double *out_p) {
    if (!c || !i || !j || !out_greater || !out_ties) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_rank(c, i, j, P, exclude_edges, out_greater, out_ties, out_cand, out_p);
    CGE_CATCH(c)
}
int cge_link_sample(cge_ctx *c, int64_t seed, int64_t stream, int64_t cap, int64_t *out_i, int64_t *out_j, double *out_p,
                    int64_t *n_edges) {
    if (!c || !n_edges) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_sample(c, seed, stream, cap, out_i, out_j, out_p, n_edges, nullptr, 0);
    CGE_CATCH(c)
}
int cge_link_auc(cge_ctx *c, int part, int nparts, int64_t *out_less, int64_t *out_ties, double *out_p, int64_t *n_neg,
                 double summary[3]) {
    if (!c || !n_neg || !summary) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_auc(c, part, nparts, out_less, out_ties, out_p, n_neg, summary);
    CGE_CATCH(c)
}
int cge_link_moments(cge_ctx *c, int diag, double *deg_out, double *deg_in, double *B, double *V, double *Cobs, int64_t *n_comm) {
    if (!c || !n_comm) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_moments(c, diag, deg_out, deg_in, B, V, Cobs, n_comm);
    CGE_CATCH(c)
}
int cge_link_triangles(cge_ctx *c, double *tri_exp, double *wed_exp, int64_t *tri_obs, int64_t *wed_obs, double summary[4]) {
    if (!c || !summary) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_triangles(c, tri_exp, wed_exp, tri_obs, wed_obs, summary);
    CGE_CATCH(c)
}
// testing hook (include/cge_hip_testing.h): the matrix Q the model half works on
int cge_link_triangles_test(void *ctx, double *Q_out, int64_t ld) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !Q_out) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_triangles_q(c, Q_out, ld);
    CGE_CATCH(c)
}
// testing hook (include/cge_hip_testing.h): the same launch with the uniforms read from a caller's matrix
int cge_link_sample_test(void *ctx, const double *U, int directed_layout, int64_t cap, int64_t *out_i, int64_t *out_j, double *out_p,
                         int64_t *n_edges) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !U || !n_edges) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_link_sample(c, 0, 0, cap, out_i, out_j, out_p, n_edges, U, directed_layout != 0);
    CGE_CATCH(c)
}

// ---- helpers ----------------------------------------------------------------------------------------
int64_t cge_idx(int64_t n, int64_t i, int64_t j) { return n * (i - 1) - (i - 1) * (i - 2) / 2 + j - i + 1; }

int cge_js(cge_ctx *c, const double *vC, const double *vB, int64_t len, const uint8_t *vI, int internal, double *out) {
    if (!c || !vC || !vB || !out || len <= 0) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_js(c, vC, vB, len, vI, internal, out);
    CGE_CATCH(c)
}

int cge_edge_scatter(cge_ctx *c, const int64_t *v_to_l, int64_t N, int64_t C, int directed, int64_t e0, int64_t e1,
                     double *wedges_out, double *vect_C_out) {
    if (!c || N <= 0 || C <= 0 || e0 < 0 || e1 < e0) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_edge_scatter(c, v_to_l, N, C, directed, e0, e1, wedges_out, vect_C_out);
    CGE_CATCH(c)
}

// ---- louvain_clust (src/clustering.jl:14-68): level-1 communities of the resident graph -------------------------------
int cge_louvain(cge_ctx *c, int64_t *comm_out, int64_t *n_comm, double *modularity, int64_t *rounds) {
    if (!c || !comm_out) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (!c->src.p || c->m <= 0 || c->n <= 0) CGE_THROW(CGE_E_ARG, "louvain: no resident graph (cge_set_graph)");
    if (c->edges_sharded) CGE_THROW(CGE_E_ARG, "louvain: the resident edge list is sharded over the ranks (option shard_ingest)");
    k_louvain_level1(c, comm_out, n_comm, modularity, rounds);
    CGE_CATCH(c)
}
// the hierarchy (src/clustering.jl:20-24: `louvain -l -1` computes every level, `hierarchy -l 1` keeps the first)
int cge_louvain_levels(cge_ctx *c, int64_t max_levels, int64_t levels_cap, int64_t *comm_out, int64_t *n_levels, int64_t *n_comm,
                       double *modularity, int64_t *rounds) {
    if (!c || !n_levels || levels_cap < 0) return CGE_E_ARG;
    if (levels_cap > 0 && (!comm_out || !n_comm || !modularity || !rounds)) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (!c->src.p || c->m <= 0 || c->n <= 0) CGE_THROW(CGE_E_ARG, "louvain: no resident graph (cge_set_graph)");
    if (c->edges_sharded) CGE_THROW(CGE_E_ARG, "louvain: the resident edge list is sharded over the ranks (option shard_ingest)");
    *n_levels = k_louvain_levels(c, max_levels, levels_cap, comm_out, n_comm, modularity, rounds);
    if (levels_cap > 0 && *n_levels > levels_cap)
        CGE_THROW(CGE_E_ARG, "louvain: the hierarchy has %lld levels, the caller's arrays hold %lld", (long long)*n_levels,
                  (long long)levels_cap);
    CGE_CATCH(c)
}

// ---- ECG: an ensemble of relabelled level-1 passes, edges reweighted by co-membership, the hierarchy on those weights ----
// the checks that need no device come first (as cge_score_batch)
static int ecg_check_args(cge_ctx *c, const cge_ecg_args *a) {
    CGE_TRY(c)
    if (a->members < 1 || a->members > 64) CGE_THROW(CGE_E_ARG, "ecg: members = %lld is outside 1 .. 64", (long long)a->members);
    if (!(a->w_min >= 0.0 && a->w_min < 1.0)) CGE_THROW(CGE_E_ARG, "ecg: w_min = %g is not in [0, 1)", a->w_min);
    if (a->final_level == 0 || a->final_level < -1)
        CGE_THROW(CGE_E_ARG, "ecg: final_level = %lld is not 1, 2, ... or -1 (the last level)", (long long)a->final_level);
    CGE_CATCH(c)
}
static void ecg_need_graph(cge_ctx *c) {
    if (!c->src.p || c->m <= 0 || c->n <= 0) CGE_THROW(CGE_E_ARG, "ecg: no resident graph (cge_set_graph)");
    if (c->edges_sharded) CGE_THROW(CGE_E_ARG, "ecg: the resident edge list is sharded over the ranks (option shard_ingest)");
}
int cge_ecg(cge_ctx *c, const cge_ecg_args *a, int64_t *comm_out, int64_t *n_comm, double *modularity, double *modularity_ecg,
            double *edge_weights_out) {
    if (!c || !a || !comm_out || !n_comm || !modularity) return CGE_E_ARG;
    if (int rc = ecg_check_args(c, a)) return rc;
    CGE_TRY_ON_DEVICE(c)
    ecg_need_graph(c);
    EcgHostOut o;
    o.comm = comm_out; o.n_comm = n_comm; o.q = modularity; o.q_ecg = modularity_ecg; o.edge_w = edge_weights_out;
    k_ecg(c, a->members, a->w_min, a->seed, a->final_level, false, o);
    CGE_CATCH(c)
}
// the testing hook (include/cge_hip_testing.h): the member and peel stages alone
int cge_ecg_members_test(void *ctx, int64_t members, int64_t seed, int64_t *members_out, int64_t *n_comm, int64_t *rounds,
                         double *modularity, int32_t *core_out) {
    cge_ctx *c = (cge_ctx *)ctx;
    const cge_ecg_args args = {members, 0.0, seed, -1}, *a = &args;
    if (!c || !members_out || !n_comm || !rounds || !modularity || !core_out) return CGE_E_ARG;
    if (int rc = ecg_check_args(c, a)) return rc;
    CGE_TRY_ON_DEVICE(c)
    ecg_need_graph(c);
    EcgHostOut o;
    o.member_comm = members_out; o.member_nc = n_comm; o.member_rounds = rounds; o.member_q = modularity; o.core = core_out;
    k_ecg(c, a->members, a->w_min, a->seed, a->final_level, true, o);
    CGE_CATCH(c)
}

// ---- options / statistics ---------------------------------------------------------------------------
int cge_set_option(cge_ctx *c, const char *key, int64_t value) {
    if (!c || !key) return CGE_E_ARG;
    const auto is = [&](const char *k) { return !strcmp(key, k); };
    const auto ranged = [&](auto &field, int64_t lo, int64_t hi) { // lo <= value <= hi, else refused
        if (value < lo || value > hi) return (int)CGE_E_ARG;
        field = (std::remove_reference_t<decltype(field)>)value;
        return (int)CGE_OK;
    };
    const auto flag = [&](auto &field) { field = value != 0; return (int)CGE_OK; };
    if (is("diameter")) return ranged(c->opt_diameter, 0, 2); // 0 auto, 1 brute force, 2 pruned only
    // point-to-reference maxima of the pruned diameter: 2 (default) bf16 matrix pipe on two-term operands (K <= 128, else as 1),
    // 1 fp32-input MFMA (both: rigorous upper bounds); 0: fp64 MFMA
    if (is("diameter_f32")) return ranged(c->opt_diameter_f32, 0, 2);
    if (is("fit_persistent")) return ranged(c->opt_fit_persistent, 0, 2); // 0 auto, 1 never, 2 whenever the score graph fits the register file
    if (is("pow_exp2")) return flag(c->opt_pow_exp2); // 1 (default): (1 - D)^alpha from log2(1 - D) kept per score; 0: the library pow per alpha
    // N > 1 only: 0 = runsplit replicated, 1 (default) = forced phase and big batches of the global phase split over the ranks,
    // 2 = every batch (tests)
    if (is("shard_runsplit")) return ranged(c->opt_shard_forced, 0, 2);
    // N > 1: 0 = tallies replicated, 1 (default) = split from 10^5 samples on with the in-library communicator, 2 = always
    if (is("shard_samples")) return ranged(c->opt_shard_samples, 0, 2);
    // exact mode beyond 8192 vertices: 1 (default) = score graph relabelled by community, 0 = as given (A/B, tests)
    if (is("exact_relabel")) return flag(c->opt_exact_relabel);
    // 1: sweeps from 256 vertices on relabel the score graph by community and sum vect_B by tiles (measured slower); 0 (default):
    // row bins + row sums + fold
    if (is("bvec_blocks")) return flag(c->opt_bvec_blocks);
    // N > 1: 1 = the N x N landmark-pair matrix is reduce-scattered by row blocks (a fetch of the landmark edge list is then
    // collective); 0 (default): all-reduced, every consumer local
    if (is("wedges_reduce_scatter")) return flag(c->opt_wedges_rs);
    // 1 (default): in landmark mode the power matrix, vect_B's tile sums and the local score's tallies ride on the launch of the
    // undirected persistent fit; 0: separate launches (A/B, cross-check)
    if (is("fit_fused")) return flag(c->opt_fit_fused);
    // N > 1: 1 = cge_set_graph keeps this rank's slice of the edge list only and cge_set_embedding uploads a slice of rows per rank
    // and all-gathers them over xGMI (set the collectives first); 0 (default): every rank uploads and keeps everything
    if (is("shard_ingest")) return flag(c->opt_shard_ingest);
    // N > 1: 1 = cge_set_embedding / cge_set_embedding_device keep the rows of this rank's communities only (sharded BY COMMUNITY;
    // set the collectives and upload the communities first); 0 (default): every rank holds every row
    if (is("shard_rows")) return flag(c->opt_shard_rows);
    // 1: cge_score also builds the landmark-pair matrix / edge count that landmarks() returns (src/landmarks.jl:433-463; the
    // undirected score itself does not read it); 0 (default): on first fetch
    if (is("landmark_edges")) return flag(c->opt_landmark_edges);
    // iterations after which a Chung-Lu fit that has not converged raises CGE_E_ASSERT (default 2 000 000)
    // an undirected exact sweep on the upper tiles of the current alpha's GD alone (about 4 N^2 bytes instead of 17.6 - 28 N^2):
    // 0 (default) = where the resident matrices would be refused, 1 = wherever the form applies (N >= 256, C >= 2, exact_relabel)
    if (is("exact_packed")) return ranged(c->opt_exact_packed, 0, 1);
    // the same form for a directed exact sweep (the model's matrix is symmetric; the fit, vect_B and the tallies read the upper
    // tiles): 0 (default) = never, refused beyond the resident limit; 1 = where the resident matrices would be refused; 2 = wherever
    // the form applies (N >= 256, C >= 2, exact_relabel).  Never a persistent fit; no effect on undirected or landmark-mode sweeps
    if (is("exact_packed_directed")) return ranged(c->opt_exact_packed_directed, 0, 2);
    if (is("fit_max_iterations")) return ranged(c->opt_fit_max_iters, 1, INT64_MAX);
    // cge_ecg: members whose rounds run in lock-step, one set of launches and one read-back per round; 0 (default) = as many as
    // the memory holds up to the built-in bound, g >= 1 = at most g.  The results do not depend on it
    if (is("ecg_group")) return ranged(c->opt_ecg_group, 0, 64);
    return CGE_E_ARG;
}
// the testing knobs (include/cge_hip_testing.h): not part of the boundary
int cge_set_test_option(void *ctx, const char *key, int64_t value) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !key) return CGE_E_ARG;
    // 1 = vect_B by the kernels of score graphs beyond the LDS budget
    if (!strcmp(key, "test_bvec_plain")) { c->opt_test_bvec_plain = value != 0; return CGE_OK; }
    // 1 = rss2 by the one-kernel walk at every width (the comparator of the chain + merge form)
    if (!strcmp(key, "test_rss2_one_kernel")) { c->opt_test_rss2_one_kernel = value != 0; return CGE_OK; }
    // which wave of a batched eigen-solver workgroup plays which role: 0 by SIMD placement, 1 identity, 2 reversed, 3 rotated by one
    if (!strcmp(key, "test_eig_roles") && value >= 0 && value <= 3) { c->opt_test_eig_roles = (int)value; return CGE_OK; }
    // the form of the bf16-split bound pass of the diameter: 0 by the number of reference points, 1 streaming, 2 register-resident
    if (!strcmp(key, "test_pcent_form") && value >= 0 && value <= 2) { c->opt_test_pcent_form = (int)value; return CGE_OK; }
    // start skew of the persistent fits' tile waves, in naps of ~3 us
    if (!strcmp(key, "fit_persistent_test_delay") && value >= 0 && value <= 100000) { c->opt_fit_test_delay = (int)value; return CGE_OK; }
    // 1 = the persistent fit abandons every launch at once
    if (!strcmp(key, "fit_persistent_test_timeout")) { c->opt_fit_test_timeout = value != 0; return CGE_OK; }
    // bytes that replace the 200e9 of the resident exact sweep's guard (0: the default)
    // Louvain levels >= 2: segments longer than this are decided by a wave (-2: the default, -1: every vertex, 2^31 - 1: none)
    if (!strcmp(key, "louvain_wave_len") && value >= -2 && value <= INT32_MAX) { c->opt_test_louvain_wave_len = value; return CGE_OK; }
    // 1 = a resident directed launch-per-iteration fit goes by the tile pair (fit_symtile_dir_kernel<false>), the comparator of the
    // packed directed sweep
    if (!strcmp(key, "fit_dir_tiles")) { c->opt_test_fit_dir_tiles = value != 0; return CGE_OK; }
    if (!strcmp(key, "exact_resident_limit") && value >= 0) { c->opt_test_resident_limit = (double)value; return CGE_OK; }
    // which groups a round of runsplit's driver (advance_heaps) puts into its batch: 0 as ever, 1 the global phase splits the top of
    // its heap alone, 2 every candidate above the threshold (no `take` cut), 3 as 0 and the forced phase's local heaps speculate too
    if (!strcmp(key, "test_lm_speculate")) {
        if (value < 0 || value > 3) return CGE_E_ARG;
        c->opt_test_lm_speculate = (int)value;
        return CGE_OK;
    }
    // the CU count every launch shape of this context is sized by (0: the device's own).  It only shrinks: the persistent fits are
    // co-resident because G <= the device's CUs
    if (!strcmp(key, "test_device_cus") && value >= 0) {
        int real = 0;
        try {
            HIP_CHECK(hipSetDevice(c->device));
            real = device_cus(c, true);
        } catch (const CgeError &e) {
            return e.code;
        }
        if (value > real) return CGE_E_ARG;
        c->opt_test_cus = (int)value;
        return CGE_OK;
    }
    return CGE_E_ARG;
}
int cge_get_stat(cge_ctx *c, const char *key, int64_t *value) {
    if (!c || !key || !value) return CGE_E_ARG;
    if (!strcmp(key, "landmarks")) *value = c->lm_ready ? c->N : 0; // no side effects (cge_landmarks_info may build the N x N matrix)
    else if (!strcmp(key, "diameter_path")) *value = c->stat_diameter_path;
    else if (!strcmp(key, "diameter_candidate_pairs")) *value = c->stat_cand_pairs;
    else if (!strcmp(key, "diameter_candidate_tiles")) *value = c->stat_cand_tiles;
    else if (!strcmp(key, "diameter_refs")) *value = c->stat_nref;
    else if (!strcmp(key, "diameter_bound_pass")) *value = c->stat_bound_pass; // of the last pruned diameter: 2 bf16-split, 1 fp32 MFMA, 0 fp64 MFMA
    else if (!strcmp(key, "diameter_arg_i")) *value = c->stat_hi_i + 1; // the arg-max pair of the last diameter (1-based vertex ids)
    else if (!strcmp(key, "diameter_arg_j")) *value = c->stat_hi_j + 1;
    else if (!strcmp(key, "fit_persistent_alphas")) *value = c->stat_fit_persistent;
    else if (!strcmp(key, "fit_iterations")) *value = c->stat_fit_iters;
    else if (!strcmp(key, "exact_packed")) *value = c->stat_exact_packed; // the last sweep ran on the packed upper tiles
    else if (!strcmp(key, "exact_matrix_bytes")) *value = c->stat_exact_matrix_bytes; // O(N^2) device bytes the last exact sweep required
    else if (!strcmp(key, "fit_fused_alphas")) *value = c->stat_fit_fused; // alphas of the last sweep whose chain rode on the fit's launch
    else if (!strcmp(key, "fit_persistent_fallbacks")) *value = c->stat_fit_fallbacks;
    else if (!strcmp(key, "fit_batched_launches")) *value = c->stat_fit_batched_launches;
    else if (!strcmp(key, "fit_batched_alphas")) *value = c->stat_fit_batched_alphas;
    else if (!strcmp(key, "landmark_batches")) *value = c->stat_lm_batches;
    else if (!strcmp(key, "landmark_batch_rows")) *value = c->stat_lm_rows;
    else if (!strcmp(key, "landmark_splits")) *value = c->stat_lm_splits;
    else if (!strcmp(key, "landmark_pops")) *value = c->stat_lm_pops;                   // groups popped by the replay, both phases
    else if (!strcmp(key, "landmark_splits_failed")) *value = c->stat_lm_failed;        // splits computed that failed, popped or not
    else if (!strcmp(key, "landmark_take_rounded")) *value = c->stat_lm_take_rounded;   // rounds whose batch the 512 rule cut down
    else if (!strcmp(key, "ecg_groups")) *value = c->stat_ecg_groups; // of the last cge_ecg: lock-step groups,
    else if (!strcmp(key, "ecg_member_rounds")) *value = c->stat_ecg_member_rounds; // rounds summed over the members,
    else if (!strcmp(key, "ecg_peel_rounds")) *value = c->stat_ecg_peel_rounds;     // rounds of the 2-core that removed a vertex,
    else if (!strcmp(key, "ecg_levels")) *value = c->stat_ecg_levels;               // levels of the final hierarchy
    else if (!strcmp(key, "link_topk_survivors")) *value = c->link.stat_survivors; // of the last cge_link_topk: pairs evaluated exactly,
    else if (!strcmp(key, "link_topk_queries")) *value = c->link.stat_queries;     // its queries
    else if (!strcmp(key, "link_rank_survivors")) *value = c->link.stat_rank_survivors; // of the last cge_link_rank: the same,
    else if (!strcmp(key, "link_rank_queries")) *value = c->link.stat_rank_queries;     // its distinct query vertices
    else if (!strcmp(key, "link_sample_edges")) *value = c->link.stat_sample_edges;         // of the last cge_link_sample: its edges,
    else if (!strcmp(key, "link_sample_survivors")) *value = c->link.stat_sample_survivors; // the pairs evaluated exactly,
    else if (!strcmp(key, "link_sample_tiles")) *value = c->link.stat_sample_tiles;         // the tiles walked
    else if (!strcmp(key, "link_auc_survivors")) *value = c->link.stat_auc_survivors; // of the last cge_link_auc: pairs evaluated exactly,
    else if (!strcmp(key, "link_auc_tiles")) *value = c->link.stat_auc_tiles;         // the tiles walked,
    else if (!strcmp(key, "link_auc_proven")) *value = c->link.stat_auc_proven;       // the pairs the filter settled alone
    else if (!strcmp(key, "link_moments_exact")) *value = c->link.stat_mom_exact; // of the last cge_link_moments: pairs through link_p,
    else if (!strcmp(key, "link_moments_fast")) *value = c->link.stat_mom_fast;   // pairs from the Gram value,
    else if (!strcmp(key, "link_moments_saturated")) *value = c->link.stat_mom_saturated; // pairs with p > 1,
    else if (!strcmp(key, "link_moments_tiles")) *value = c->link.stat_mom_tiles;         // the tiles walked
    else if (!strcmp(key, "link_tri_tiles")) *value = c->link.stat_tri_tiles; // of the last cge_link_triangles: 128 x 128 tiles walked,
    else if (!strcmp(key, "link_tri_saturated")) *value = c->link.stat_tri_saturated;     // pairs i < j with p > 1,
    else if (!strcmp(key, "link_tri_matrix_bytes")) *value = c->link.stat_tri_bytes;      // the bytes of Q
    else if (!strcmp(key, "cut_tie_tasks")) { // (read from the device on request: a synchronising copy)
        int v = 0;
        if (c->cut_ties.p && (hipStreamSynchronize(c->stream) != hipSuccess ||
                              hipMemcpy(&v, c->cut_ties.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
            return CGE_E_HIP;
        *value = v;
    }
    else if (!strcmp(key, "edge_layout_build_us")) *value = c->stat_layout_build_us;
    else if (!strcmp(key, "edge_chunks")) *value = c->be_nchunks;
    else if (!strcmp(key, "edges_resident")) *value = c->m;
    else if (!strcmp(key, "edges_total")) *value = c->m_total;
    else if (!strcmp(key, "embedding_words_resident")) *value = (i64)c->Xr.n;
    else if (!strcmp(key, "rows_resident")) *value = c->Xr.p ? lm_rows(c) : 0; // embedding rows held by this rank (option shard_rows: ~ n / world)
    else if (!strcmp(key, "rows_total")) *value = c->n;
    else if (!strcmp(key, "collective_calls")) *value = c->stat_coll_calls;
    else if (!strcmp(key, "collective_bytes")) *value = c->stat_coll_bytes;
    else if (!strcmp(key, "diameter_bits")) memcpy(value, &c->stat_last_hi, sizeof(double)); // bit pattern of the last `hi`
    else return CGE_E_ARG;
    return CGE_OK;
}

// ---- profiling --------------------------------------------------------------------------------------
int cge_profile_enable(cge_ctx *c, int on) {
    if (!c) return CGE_E_ARG;
    c->profiling = on != 0;
    return CGE_OK;
}
int cge_profile_select(cge_ctx *c, const char *names) {
    if (!c) return CGE_E_ARG;
    c->profile_only.clear();
    std::string cur;
    for (const char *p = names ? names : ""; ; p++) {
        if (*p == ',' || *p == 0) {
            if (!cur.empty()) c->profile_only.push_back(cur);
            cur.clear();
            if (*p == 0) break;
        } else
            cur.push_back(*p);
    }
    return CGE_OK;
}
int cge_profile_reset(cge_ctx *c) {
    if (!c) return CGE_E_ARG;
    flush_timers(c);
    c->timers.clear();
    return CGE_OK;
}
int cge_profile_get(cge_ctx *c, const char *name, int64_t *launches, double *total_ms) {
    if (!c || !name) return CGE_E_ARG;
    flush_timers(c);
    auto it = c->timers.find(name);
    if (launches) *launches = it == c->timers.end() ? 0 : it->second.launches;
    if (total_ms) *total_ms = it == c->timers.end() ? 0.0 : it->second.total_ms;
    return CGE_OK;
}
int cge_profile_names(cge_ctx *c, char *buf, int64_t buf_len) {
    return !c || !buf || buf_len <= 0 ? CGE_E_ARG : key_names(c->timers, buf, buf_len);
}
int cge_phase_names(cge_ctx *c, char *buf, int64_t buf_len) {
    return !c || !buf || buf_len <= 0 ? CGE_E_ARG : key_names(c->phases.ms, buf, buf_len);
}
int cge_phase_ms(cge_ctx *c, const char *phase, double *ms) {
    if (!c || !phase || !ms) return CGE_E_ARG;
    auto it = c->phases.ms.find(phase);
    *ms = it == c->phases.ms.end() ? 0.0 : it->second;
    return CGE_OK;
}

// ---- host-only test hooks (include/cge_hip_testing.h) ------------------------------------------------
int cge_host_eig_top(const double *A, int64_t d, double *v) {
    if (!A || !v || d <= 0) return CGE_E_ARG;
    host_eig_top(A, d, v);
    return CGE_OK;
}
// the launch groups of a batch's members, undirected or directed: flow_batch_member picks them, batch_group_closes packs them
static int batch_pack(const int64_t *N, int64_t K, int cus, bool directed, int32_t *group_of) {
    if (!N || !group_of || K < 0 || cus <= 0) return CGE_E_ARG;
    int groups = 0, g_sum = 0, g_nw = 0, g_size = 0;
    for (i64 k = 0; k < K; k++) {
        FlowGeometry g;
        if (!flow_batch_member(N[k], cus, directed, &g)) { group_of[k] = -1; continue; } // (sequential)
        if (g_size == 0 || batch_group_closes(g_sum, g_nw, g_size, g.G, g.NW, cus)) { groups++; g_sum = 0; g_size = 0; }
        g_sum += g.G; g_nw = g.NW; g_size++;
        group_of[k] = groups - 1;
    }
    return groups;
}
int cge_batch_pack_test(const int64_t *N, int64_t K, int cus, int32_t *group_of) { return batch_pack(N, K, cus, false, group_of); }
int cge_batch_pack_dir_test(const int64_t *N, int64_t K, int cus, int32_t *group_of) { return batch_pack(N, K, cus, true, group_of); }
// host-only hooks (include/cge_hip_testing.h): the persistent fits' one geometry and one slot layout
int cge_fit_dir_geometry_test(int64_t N, int cus, int *applies, int *G, int *NW, int *NSB) {
    if (!applies || !G || !NW || !NSB) return CGE_E_ARG;
    FlowGeometry g;
    *applies = flow_geometry(N, cus, &g) ? 1 : 0;
    if (*applies) { *G = g.G; *NW = g.NW; *NSB = g.NSB; }
    return CGE_OK;
}
int cge_fit_slots_test(int64_t N, int directed, int64_t out[5]) {
    if (!out || N <= 0 || N > 64 * 64) return CGE_E_ARG;
    const int Nt = (int)((N + 63) / 64);
    const FlowSlots s = flow_slots(Nt, (i64)Nt * 64, directed != 0);
    out[0] = s.sync; out[1] = s.ring; out[2] = s.fq; out[3] = s.P; out[4] = s.doubles;
    return CGE_OK;
}
int cge_host_pos_draw(int64_t seed, int64_t stream_id, int64_t S, int64_t m, int64_t *pos_idx) {
    if (!pos_idx || S <= 0 || m <= 0) return CGE_E_ARG;
    host_pos_draw(seed, stream_id, S, m, pos_idx);
    return CGE_OK;
}
int cge_group_eig(void *ctx, const double *A, int64_t T, int64_t d, double *v) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !A || !v || T <= 0 || d <= 0 || d > 512) return CGE_E_ARG;
    CGE_TRY(c)
    DevBuf<double> dA, dv;
    dA.ensure((size_t)T * d * d);
    dv.ensure((size_t)T * d);
    HIP_CHECK(hipMemcpyAsync(dA.p, A, sizeof(double) * T * d * d, hipMemcpyHostToDevice, c->stream));
    k_group_eig(c, dA.p, T, d, dv.p);
    HIP_CHECK(hipMemcpyAsync(v, dv.p, sizeof(double) * T * d, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the statistics stage of a split and the side sums, for caller-supplied groups
int cge_group_stats_test(void *ctx, const int32_t *ids, const int32_t *task_row_off, int64_t T, const uint8_t *side, const double *mean_in,
                         double *mean, double *sw, double *cov, double *vec, double *z, double *sums) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !ids || !task_row_off || T <= 0 || !mean || !cov || !vec || !z || (!mean_in && !sw) || (side && !sums)) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_group_stats_test(c, ids, task_row_off, T, side, mean_in, mean, sw, cov, vec, z, sums);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the cut stage of a split on caller-supplied projections
int cge_group_cut_test(void *ctx, const int32_t *ids, const int32_t *task_row_off, int64_t T, int method, const double *z, int force_generic,
                       int32_t *rc, int32_t *nlow, int32_t *children, double *vlow, double *vhigh, double *cmeans, int32_t *route,
                       int32_t *ties) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !ids || !task_row_off || T <= 0 || !rc || !nlow || !children || !vlow || !vhigh || !cmeans || !route || !ties) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_group_cut_test(c, ids, task_row_off, T, method, z, force_generic, rc, nlow, children, vlow, vhigh, cmeans, route, ties);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the gather and one bound pass of the pruned diameter
int cge_diameter_bounds_test(void *ctx, const int64_t *v2l, int64_t N, const int64_t *lcomm, int64_t C, int pass, double *P,
                             int64_t *nref, int *pass_ran, double *ref_points, double *mean) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !v2l || !lcomm || !P || !nref || !pass_ran || N <= 0 || C <= 0 || pass < 0 || pass > 2) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_diameter_bounds_test(c, v2l, N, lcomm, C, pass, P, nref, pass_ran, ref_points, mean);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the squared distances of caller-supplied reference points, as the diameter forms them
int cge_ref_dist2_test(void *ctx, const double *refs, int64_t nref, double *rd2, double *mean) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !refs || !rd2 || nref <= 0) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_ref_dist2_test(c, refs, nref, rd2, mean);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): aggregate, landmark-pair matrix and degrees of a caller's assignment
int cge_landmark_graph_test(void *ctx, cge_landmark_graph_io *io) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !io || !io->v2l || io->N <= 0 || io->wedge_form < 0 || io->wedge_form > 2) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_landmark_graph_test(c, io);
    CGE_CATCH(c)
}
// host-only hook (include/cge_hip_testing.h): the tiled form's geometry, as k_wedge_scatter_blocked reads it
int cge_wedge_geometry_test(int64_t N, int weighted, int64_t n_chunks, int *applies, int *rshift, int *colbits, int64_t *ntile,
                            int64_t *lds_pass1, int64_t *lds_pass2) {
    if (!applies || !rshift || !colbits || !ntile || !lds_pass1 || !lds_pass2) return CGE_E_ARG;
    WedgeGeometry G;
    *applies = k_wedge_geometry(N, weighted ? 8 : 4, n_chunks, &G) ? 1 : 0;
    if (!*applies) return CGE_OK;
    *rshift = G.rshift; *colbits = G.colbits; *ntile = G.ntile;
    *lds_pass1 = (int64_t)G.lds1; *lds_pass2 = (int64_t)G.lds2;
    return CGE_OK;
}

int cge_pow_test(void *ctx, const double *x, int64_t n, double alpha, int method, double *out) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !x || !out || n <= 0) return CGE_E_ARG;
    CGE_TRY(c)
    k_pow_test(c, x, n, alpha, method, out);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the packed form's extrema pass and generator on a caller's embedding
int cge_packed_gd_test(void *ctx, const double *emb, const double *diag, int64_t N, int64_t d, double alpha, int pow_method,
                       double *lo_hi, double *GD) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !emb || !diag || !lo_hi || !GD || N <= 0 || d <= 0 || (pow_method != 0 && pow_method != 1)) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_packed_gd_test(c, emb, diag, N, d, alpha, pow_method, lo_hi, GD);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): vect_B by one named form of the sweep, and its divergence by the device-side modes
int cge_vect_b_test(void *ctx, const cge_vect_b_problem *p, const cge_vect_b_problem *p2, int directed, int form, int landmarks,
                    int n_modes, int *form_ran) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !p || !form_ran || form < 0 || form > 7 || n_modes < 1 || n_modes > 2) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_vect_b_test(c, p, p2, directed != 0, form, landmarks, n_modes, form_ran);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): one Chung-Lu fit from a caller's start by one named form of the sweep
int cge_fit_test(void *ctx, cge_fit_problem *problems, int n_problems, int directed, int form, double eps, double delta, int *form_ran) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !problems || !form_ran || form < 0 || form > 8 || n_problems < 1) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_fit_test(c, problems, n_problems, directed != 0, form, eps, delta, form_ran);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): one alpha of the fused chain -- the fit with its epilogue's outputs, the bins, the divergence
int cge_fused_chain_test(void *ctx, cge_fused_chain_problem *problems, int n_problems, int directed, double eps, double delta) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !problems || n_problems < 1) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (directed) CGE_THROW(CGE_E_ARG, "fused_chain_test: the fused chain is undirected only");
    host_fused_chain_test(c, problems, n_problems, eps, delta);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the set-up of an alpha sweep -- degrees, layout, D, extrema, logarithm, start vectors
int cge_sweep_setup_test(void *ctx, cge_sweep_setup_io *io) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !io) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_sweep_setup_test(c, io);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the local score's sampler, prepared pairs, pair distances and tallies, stage by stage
int cge_local_score_test(void *ctx, cge_local_score_io *io) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !io || io->form < 0 || io->form > 5 || io->draw_route < 0 || io->draw_route > 2) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    host_local_score_test(c, io);
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the per-group stable sort of the projections as runsplit calls it
int cge_segment_sort_test(void *ctx, const double *z, const int32_t *task_row_off, int64_t T, double *zs_out, int32_t *perm_out) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !z || !task_row_off || !zs_out || !perm_out || T <= 0) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    const i64 R = task_row_off[T];
    if (R <= 0) CGE_THROW(CGE_E_ARG, "segment_sort_test: no rows");
    std::vector<i32> rt(R), rows(R);
    i64 max_len = 0;
    for (i64 t = 0; t < T; t++) {
        if (task_row_off[t + 1] <= task_row_off[t]) CGE_THROW(CGE_E_ARG, "segment_sort_test: empty group");
        max_len = std::max<i64>(max_len, task_row_off[t + 1] - task_row_off[t]);
        for (i64 j = task_row_off[t]; j < task_row_off[t + 1]; j++) { rt[j] = (i32)t; rows[j] = (i32)j; }
    }
    DevBuf<double> dz, dzs;
    DevBuf<i32> dtro, drt, drows, dperm, dsrows, dstatus;
    dz.ensure(R); dzs.ensure(R); dtro.ensure(T + 1); drt.ensure(R); drows.ensure(R); dperm.ensure(R); dsrows.ensure(R); dstatus.ensure(T);
    HIP_CHECK(hipMemcpyAsync(dz.p, z, sizeof(double) * R, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(dtro.p, task_row_off, sizeof(i32) * (T + 1), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(drt.p, rt.data(), sizeof(i32) * R, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(drows.p, rows.data(), sizeof(i32) * R, hipMemcpyHostToDevice, c->stream));
    k_segmented_sort_z(c, dz.p, drows.p, drt.p, dtro.p, R, T, dzs.p, dperm.p, dsrows.p, dstatus.p, max_len);
    HIP_CHECK(hipMemcpyAsync(zs_out, dzs.p, sizeof(double) * R, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(perm_out, dperm.p, sizeof(i32) * R, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): lane 0's sum of 64 values per row by the shfl_down tree and by the VALU lane
// swaps that replace it in the projection kernel -- the same bits are expected
int cge_wave_tree_test(void *ctx, const double *x, int64_t n_rows, double *out_ref, double *out_new) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !x || !out_ref || !out_new || n_rows <= 0) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    DevBuf<double> dx, da, db;
    dx.ensure((size_t)n_rows * 64); da.ensure(n_rows); db.ensure(n_rows);
    HIP_CHECK(hipMemcpyAsync(dx.p, x, sizeof(double) * n_rows * 64, hipMemcpyHostToDevice, c->stream));
    k_wave_tree_test(c, dx.p, n_rows, da.p, db.p);
    HIP_CHECK(hipMemcpyAsync(out_ref, da.p, sizeof(double) * n_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(out_new, db.p, sizeof(double) * n_rows, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the resident row-major matrix itself, so that the tests of the embedding views compare
// every element and not a score
int cge_resident_embedding_test(void *ctx, double *out, int64_t capacity_doubles, int64_t *rows, int64_t *d, int32_t *ids_out) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !rows || !d) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    if (!c->Xr.p || c->d <= 0) CGE_THROW(CGE_E_ARG, "embedding not resident");
    const i64 nl = lm_rows(c);
    *rows = nl;
    *d = c->d;
    if (!out || capacity_doubles < nl * c->d) CGE_THROW(CGE_E_ARG, "resident embedding: %lld x %lld doubles do not fit the buffer", (long long)nl, (long long)c->d);
    HIP_CHECK(hipMemcpyAsync(out, c->Xr.p, sizeof(double) * (size_t)nl * c->d, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (ids_out)
        for (i64 i = 0; i < nl; i++) ids_out[i] = c->rows_sharded ? c->h_loc2glob[i] : (i32)i;
    CGE_CATCH(c)
}

// testing hook (include/cge_hip_testing.h): the resident graph and vertex data themselves, copied from the DEVICE tables
int cge_resident_graph_test(void *ctx, cge_resident_graph *o) {
    cge_ctx *c = (cge_ctx *)ctx;
    if (!c || !o) return CGE_E_ARG;
    CGE_TRY_ON_DEVICE(c)
    const bool graph = c->src.p && c->dst.p && c->m > 0;
    o->n = c->n;
    o->m = graph ? c->m : 0;
    o->unit = graph && c->unit_weights ? 1 : 0;
    o->n_comm_max = c->comm.p ? c->n_comm_max : 0;
    o->n_comm16 = c->comm16.p ? (i64)c->comm16.n : 0;
    o->have = (c->comm.p ? 1 : 0) | (c->vw.p ? 2 : 0);
    const size_t m = (size_t)o->m, n = (size_t)c->n;
    if (((o->src || o->dst || o->w) && o->cap_edges < o->m) || ((o->comm || o->vweight) && o->cap_vertices < o->n) ||
        (o->comm16 && o->cap_comm16 < o->n_comm16))
        CGE_THROW(CGE_E_ARG, "resident graph: n = %lld, m = %lld, %lld comm16 entries do not fit the buffers", (long long)o->n,
                  (long long)o->m, (long long)o->n_comm16);
    if (o->src && m) HIP_CHECK(hipMemcpyAsync(o->src, c->src.p, sizeof(i32) * m, hipMemcpyDeviceToHost, c->stream));
    if (o->dst && m) HIP_CHECK(hipMemcpyAsync(o->dst, c->dst.p, sizeof(i32) * m, hipMemcpyDeviceToHost, c->stream));
    if (o->w && m && !o->unit) {
        if (!c->w.p || c->h_w.size() != m) CGE_THROW(CGE_E_ARG, "resident graph: a weighted list without its weights or their host mirror");
        HIP_CHECK(hipMemcpyAsync(o->w, c->w.p, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    }
    if (o->comm && c->comm.p) HIP_CHECK(hipMemcpyAsync(o->comm, c->comm.p, sizeof(i32) * n, hipMemcpyDeviceToHost, c->stream));
    if (o->comm16 && c->comm16.p)
        HIP_CHECK(hipMemcpyAsync(o->comm16, c->comm16.p, sizeof(unsigned short) * c->comm16.n, hipMemcpyDeviceToHost, c->stream));
    if (o->vweight && c->vw.p) HIP_CHECK(hipMemcpyAsync(o->vweight, c->vw.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    CGE_CATCH(c)
}

} // extern "C"
