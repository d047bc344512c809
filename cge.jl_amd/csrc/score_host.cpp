// score_host.cpp -- the landmark phase's driver and the score, in stages.
// A landmark run (cge_landmarks_run, cge_score in landmark mode): lm_clamp -> lm_split -> lm_aggregate -> lm_scatter over one
// LandmarkRun.  cge_score: score_graph_landmarks | score_graph_exact -> score_samples -> the sweep; in landmark mode the local
// score's sample draw is enqueued between lm_clamp and lm_split.  cge_wgcl (everything as host arrays): wgcl_upload_score_graph
// -> wgcl_original_graph -> wgcl_samples -> the sweep.  Every exchange between ranks goes through collectives.cpp.
#include "common.hpp"
#include "../../include/cge_hip_testing.h"

// ---- shares of the ranks ------------------------------------------------------------------------------------------------------
// This rank's share of the edges: of a replicated list its slice [lo(cnt), hi(cnt)) of the edges or chunks; of a sharded list
// (and without collectives) all that it holds.
struct EdgeShare {
    i64 rank, world;
    i64 lo(i64 cnt) const { return cnt * rank / world; }
    i64 hi(i64 cnt) const { return cnt * (rank + 1) / world; }
};
static EdgeShare edge_share(const cge_ctx *c) {
    const bool split = c->has_coll && !c->edges_sharded;
    return {split ? c->coll.rank : 0, split ? c->coll.world : 1};
}
// the row block [r0, r1) of the N x N landmark-pair matrix this rank ends up with after a reduce-scatter: equal blocks of `per` rows
struct RowBlock { i64 per, r0, r1; };
static RowBlock row_block_of(i64 N, i64 rank, i64 world) {
    const i64 per = (N + world - 1) / world, r0 = std::min<i64>(N, per * rank);
    return {per, r0, std::min<i64>(N, r0 + per)};
}
static RowBlock wedge_row_block(const cge_ctx *c, i64 N) {
    return c->has_coll ? row_block_of(N, c->coll.rank, c->coll.world) : RowBlock{N, 0, N};
}

// ---- the unique-row clamp -----------------------------------------------------------------------------------------------------
// `size(unique(embedding, dims=1), 1)` (src/landmarks.jl:371-376).  Equal rows have equal hashes, so #distinct hashes <= #unique
// rows: once `land` distinct hashes are seen no clamp can apply; otherwise the rows are counted exactly on the host.  Both forms
// below return `land` in the first case and the exact count in the second.

// bitwise-distinct rows among the listed rows of the host array X (d columns): sorted by memcmp, the changes counted
static i64 count_distinct_rows(const double *X, i64 d, std::vector<i64> &rows) {
    const size_t bytes = sizeof(double) * d;
    std::sort(rows.begin(), rows.end(), [&](i64 a, i64 b) { return memcmp(X + a * d, X + b * d, bytes) < 0; });
    i64 uniq = rows.empty() ? 0 : 1;
    for (size_t t = 1; t < rows.size(); t++)
        if (memcmp(X + rows[t - 1] * d, X + rows[t] * d, bytes) != 0) uniq++;
    return uniq;
}
// `land` distinct hashes among a prefix of the rows already prove `land` distinct rows: hash 8*land rows first, the whole matrix
// only when that prefix does not settle it.  The distinct hashes are counted on the device (a set of atomicCAS slots): one
// 8-byte read-back instead of the hashes themselves and a host set.
static i64 unique_rows_local(cge_ctx *c, i64 land) {
    const i64 n = c->n, d = c->d;
    i64 done = 0;
    for (int pass = 0; pass < 2 && done < n; pass++) {
        const i64 upto = pass == 0 ? std::min<i64>(n, 8 * land) : n;
        k_row_hash(c, c->Xr.p + done * d, c->uniq_hash.p + done, upto - done, d);
        if (k_count_distinct(c, c->uniq_hash.p, upto) >= land) return land;
        done = upto;
    }
    std::vector<i64> ix(n);
    for (i64 i = 0; i < n; i++) ix[i] = i;
    cge_ensure_host_embedding(c);
    return count_distinct_rows(c->h_Xr.data(), d, ix);
}
// option shard_rows: every rank hashes its rows, the hashes are gathered by vertex id (8 bytes per vertex) and every rank counts
// the distinct ones; only if that leaves the clamp open are the rows with a shared hash -- the only candidates for equal rows --
// gathered and compared bit for bit
static i64 unique_rows_sharded(cge_ctx *c, i64 land) {
    const i64 n = c->n, d = c->d, nl = c->n_loc;
    DevBuf<uint64_t> hl;
    hl.ensure(nl);
    k_row_hash(c, c->Xr.p, hl.p, nl, d);
    HIP_CHECK(hipMemsetAsync(c->uniq_hash.p, 0, sizeof(uint64_t) * n, c->stream));
    k_scatter_u64(c, hl.p, c->loc2glob.p, nl, c->uniq_hash.p);
    cge_allreduce_dev(c, reinterpret_cast<double *>(c->uniq_hash.p), n, 2);
    if (k_count_distinct(c, c->uniq_hash.p, n) >= land) return land;
    std::vector<uint64_t> hh(n);
    HIP_CHECK(hipMemcpyAsync(hh.data(), c->uniq_hash.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<uint64_t> hs(hh);
    std::sort(hs.begin(), hs.end());
    std::vector<i32> lidx; // the rows (owner's local ids) whose hash is shared; rows of different hashes differ
    for (i64 i = 0; i < n; i++)
        if (std::upper_bound(hs.begin(), hs.end(), hh[i]) - std::lower_bound(hs.begin(), hs.end(), hh[i]) > 1) lidx.push_back(c->h_glob2loc[i]);
    const i64 nd = (i64)lidx.size();
    if (nd == 0) return n;
    DevBuf<i32> didx;
    DevBuf<double> rows;
    didx.ensure(nd);
    rows.ensure((size_t)nd * d);
    HIP_CHECK(hipMemcpyAsync(didx.p, lidx.data(), sizeof(i32) * nd, hipMemcpyHostToDevice, c->stream));
    k_gather_rows_f64(c, c->Xr.p, nl, d, 1, didx.p, nd, rows.p);
    cge_allreduce_dev(c, rows.p, nd * d, 2);
    std::vector<double> hr((size_t)nd * d);
    HIP_CHECK(hipMemcpyAsync(hr.data(), rows.p, sizeof(double) * nd * d, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<i64> q(nd);
    for (i64 t = 0; t < nd; t++) q[t] = t;
    return n - nd + count_distinct_rows(hr.data(), d, q);
}
static i64 clamp_to_unique_rows(cge_ctx *c, i64 land, int *truncated) {
    *truncated = 0;
    if (land <= 1) return land;
    c->uniq_hash.ensure(c->n);
    const i64 uniq = c->rows_sharded ? unique_rows_sharded(c, land) : unique_rows_local(c, land);
    *truncated = land > uniq;
    return std::min(land, uniq);
}

// ---- the per-edge scatters of the resident graph ------------------------------------------------------------------------------
// vect_C of the resident graph (src/divergence.jl:59-63 / :337-345 on the original edges): the blocked two-pass form
// (kernels_scatter.hip) where it applies, else the gather + atomics kernel; this rank's share, then the all-reduce
static void scatter_vectC_resident(cge_ctx *c, i64 C, int directed, double *vectC) {
    const i64 vlen = directed ? C * C : packed_len(C);
    const EdgeShare mine = edge_share(c);
    bool done = false;
    if (k_edge_scatter_blocked_applies(c, C) && (c->blocked_ready || k_build_blocked_edges(c))) {
        k_edge_scatter_blocked(c, mine.lo(c->be_nchunks), mine.hi(c->be_nchunks), C, directed, vectC);
        done = true;
    } else if (C > 1 && C <= 16384 && (c->blocked_ready || (k_blocked_edges_possible(c) && k_build_blocked_edges(c)))) {
        // beyond the 2048 row counters of the row-bucketed form: the community pairs as a dense C x C matrix through the
        // TILED two-pass form of the landmark-pair matrix (tiles of rows in LDS, written whole), then packed
        DevBuf<i64> &cnt = c->wed_cnt;
        cnt.ensure(1);
        double *dense = vectC;
        if (!directed) { c->cc_dense.ensure((size_t)C * C); dense = c->cc_dense.p; }
        if (k_wedge_scatter_blocked(c, c->comm.p, C, mine.lo(c->be_nchunks), mine.hi(c->be_nchunks), directed, dense, cnt.p, "edge_scatter")) {
            if (!directed) k_pack_upper(c, dense, C, vectC);
            done = true;
        }
    }
    if (!done) {
        HIP_CHECK(hipMemsetAsync(vectC, 0, sizeof(double) * vlen, c->stream));
        k_edge_scatter(c, c->src.p, c->dst.p, c->unit_weights ? nullptr : c->w.p, mine.lo(c->m), mine.hi(c->m), nullptr, c->comm.p, 1, C,
                       directed, nullptr, vectC);
    }
    if (c->has_coll) cge_allreduce_dev(c, vectC, vlen, 0);
}

// One share of the edges summed into a full N x N landmark-pair matrix: the tiled two-pass form on the blocked copy of the edge
// list (kernels_scatter.hip: the tiles are written whole and *cnt counts the positive entries on the way) -- else the gather +
// atomics kernel into a zeroed matrix, which leaves *cnt alone.  form 0: the tiled form where it applies; 2: the gather form
// (the testing hook names it).  Returns whether the tiled form ran.
static bool scatter_wedges_share(cge_ctx *c, const i32 *v2l, i64 N, int directed, const EdgeShare &mine, int form, double *wedges,
                                 i64 *cnt) {
    const bool tiled = form != 2 && (c->blocked_ready || (k_blocked_edges_possible(c) && k_build_blocked_edges(c))) &&
                       k_wedge_scatter_blocked(c, v2l, N, mine.lo(c->be_nchunks), mine.hi(c->be_nchunks), directed, wedges, cnt);
    if (!tiled) {
        HIP_CHECK(hipMemsetAsync(wedges, 0, sizeof(double) * N * N, c->stream));
        k_edge_scatter(c, c->src.p, c->dst.p, c->unit_weights ? nullptr : c->w.p, mine.lo(c->m), mine.hi(c->m), v2l, c->comm.p, N,
                       c->n_comm_max, directed, wedges, nullptr);
    }
    return tiled;
}

// the landmark-pair matrix (src/landmarks.jl:433-451) and its positive-entry count
static void scatter_wedges(cge_ctx *c, int directed) {
    const i64 N = c->N;
    hipStream_t st = c->stream;
    const RowBlock blk = wedge_row_block(c, N);
    const i64 Npad = c->has_coll ? blk.per * c->coll.world : N; // (padding rows behind row N: zeros)
    c->wedges.ensure((size_t)Npad * N);
    c->wedges_block_only = false;
    DevBuf<i64> &cnt = c->wed_cnt;
    cnt.ensure(1);
    const bool tiled = scatter_wedges_share(c, c->v2l.p, N, directed, edge_share(c), 0, c->wedges.p, cnt.p);
    if (c->has_coll) {
        // every rank has summed ITS edges into a full N x N matrix.  Option "wedges_reduce_scatter" (default 0): the sums over
        // the ranks are all-reduced, after which every consumer -- cge_landmarks_fetch on ONE rank included -- is local.  With it
        // they go out BY ROW BLOCK: rank r ends with rows [per r, per (r + 1)); the consumers then work on blocks
        // (the count below, the directed score's degrees), and a fetch of the edge list is COLLECTIVE (every rank must call it:
        // the blocks are all-gathered).  Where the exchange layer has no reduce-scatter: the all-reduce.
        if (Npad > N) HIP_CHECK(hipMemsetAsync(c->wedges.p + (size_t)N * N, 0, sizeof(double) * (size_t)(Npad - N) * N, st));
        c->wedges_block_only = c->opt_wedges_rs && cge_reduce_scatter_dev(c, c->wedges.p, blk.per * N);
        if (!c->wedges_block_only) cge_allreduce_dev(c, c->wedges.p, N * N, 0);
        k_compact_count(c, c->wedges.p, N, directed, cnt.p, blk.r0, blk.r1);
        cge_allreduce_dev(c, reinterpret_cast<double *>(cnt.p), 1, 2); // (integer sum of the ranks' counts)
    } else if (!tiled)
        k_compact_count(c, c->wedges.p, N, directed, cnt.p);
    HIP_CHECK(hipMemcpyAsync(&c->n_ledges, cnt.p, sizeof(i64), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    c->wedges_ready = true;
}

// ---- the landmark run ---------------------------------------------------------------------------------------------------------
static void lm_clamp(cge_ctx *c, LandmarkRun &R) {
    check_resident(c, "landmarks");
    if (R.method < 0 || R.method > 3) CGE_THROW(CGE_E_ARG, "unknown split method %d", R.method);
    R.t0 = now_ms();
    R.land = clamp_to_unique_rows(c, R.land, &c->lm_truncated);
    c->phases.ms["lm_unique"] = now_ms() - R.t0;
}

static void lm_split(cge_ctx *c, LandmarkRun &R) {
    std::vector<i64> gid;
    host_runsplit(c, R.cl_flat, R.cl_off, R.ncl, R.land, R.forced, R.method, gid, true);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->phases.ms["landmarks"] = now_ms() - R.t0;
    c->N = (i64)c->h_mem_off.size() - 1; // every group is non-empty
    c->h_v2l.clear();                    // v_to_l (:379) is read back from the device by landmarks_fetch
}

// centroids, weights, d_ii and communities (c->lemb, lweight, dii, lcomm) of the N landmarks of the device index c->lm_memoff /
// c->lm_mem over the rows this rank holds
static void aggregate_landmarks(cge_ctx *c, i64 N) {
    const i64 d = c->d;
    c->lemb.ensure((size_t)N * d);
    c->lweight.ensure(N); c->dii.ensure(N); c->lcomm.ensure(N);
    ScopedKernelTimer tm(c, "landmark_aggregate");
    k_landmark_aggregate(c, c->Xr.p, lm_vw(c), lm_comm(c), c->lm_memoff.p, c->lm_mem.p, N, d, c->lemb.p, c->lweight.p, c->dii.p,
                         c->lcomm.p);
}

static void lm_aggregate(cge_ctx *c, LandmarkRun &R) {
    R.t0 = now_ms();
    const i64 N = c->N, d = c->d;
    aggregate_landmarks(c, N);
    if (c->rows_sharded) {
        // option shard_rows: a landmark's members live on one rank, which has just aggregated it (the others wrote zeros for
        // it); centroids, weights, d_ii and communities of ALL landmarks on every rank by one gather (N (d + 3) words)
        DevBuf<double> &X = c->samp_xchg;
        const i64 words = N * (d + 3);
        X.ensure(words);
        k_pack_landmarks(c, c->lemb.p, c->lweight.p, c->dii.p, c->lcomm.p, N, d, X.p, 0);
        cge_allreduce_dev(c, X.p, words, 2);
        k_pack_landmarks(c, c->lemb.p, c->lweight.p, c->dii.p, c->lcomm.p, N, d, X.p, 1);
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->phases.ms["aggregate"] = now_ms() - R.t0;
}

// vect_C (C x C cluster pairs, from the original edges: every landmark lies in one community, so this equals the reference's sum
// over landmark edges, src/divergence.jl:59-63) is what the score needs; the N x N landmark-pair matrix only feeds
// landmarks_fetch and the directed score's degrees.
static void lm_scatter(cge_ctx *c, LandmarkRun &R) {
    R.t0 = now_ms();
    const i64 C = c->n_comm_max;
    c->vectC.ensure(R.directed ? C * C : packed_len(C));
    scatter_vectC_resident(c, C, R.directed, c->vectC.p);
    c->lm_directed = R.directed;
    c->wedges_ready = false;
    c->n_ledges = -1;
    if (R.need_wedges) scatter_wedges(c, R.directed);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->phases.ms["scatter"] = now_ms() - R.t0;
    c->lm_ready = true;
}

void host_landmarks_run(cge_ctx *c, LandmarkRun R) {
    lm_clamp(c, R);
    lm_split(c, R);
    lm_aggregate(c, R);
    lm_scatter(c, R);
}

LandmarkRun score_landmark_run(const cge_ctx *c, const cge_score_args *a) {
    return {a->clusters_flat, a->clusters_off, a->n_clusters, a->land, a->forced, a->method, a->directed,
            a->directed != 0 || c->opt_landmark_edges != 0}; // (the undirected score itself does not read the landmark-pair matrix)
}

// the landmark-pair matrix of the last run, built on first demand (the score path skips it)
void host_landmarks_info(cge_ctx *c, const char *who) {
    if (!c->lm_ready) CGE_THROW(CGE_E_ARG, "%s: run cge_landmarks_run first", who);
    if (!c->wedges_ready) scatter_wedges(c, c->lm_directed);
}

void host_landmarks_fetch(cge_ctx *c, double *dii, double *embed, int64_t *cluster, int64_t *ledges, double *lw_e, double *lweight,
                          int64_t *v_to_l) {
    host_landmarks_info(c, "landmarks_fetch");
    if ((ledges || lw_e) && c->wedges_block_only) { // the row blocks of a reduce-scattered matrix are all-gathered in place
        cge_allgather_dev(c, c->wedges.p, wedge_row_block(c, c->N).per * c->N);
        c->wedges_block_only = false;
    }
    const i64 N = c->N, d = c->d, n = c->n;
    hipStream_t st = c->stream;
    if (dii) HIP_CHECK(hipMemcpyAsync(dii, c->dii.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (lweight) HIP_CHECK(hipMemcpyAsync(lweight, c->lweight.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    std::vector<double> rm(embed ? (size_t)N * d : 0), we(ledges || lw_e ? (size_t)N * N : 0);
    std::vector<i32> lc(cluster ? N : 0);
    if (embed) HIP_CHECK(hipMemcpyAsync(rm.data(), c->lemb.p, sizeof(double) * N * d, hipMemcpyDeviceToHost, st));
    if (cluster) HIP_CHECK(hipMemcpyAsync(lc.data(), c->lcomm.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
    if (ledges || lw_e) HIP_CHECK(hipMemcpyAsync(we.data(), c->wedges.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (embed)
        for (i64 l = 0; l < N; l++)
            for (i64 k = 0; k < d; k++) embed[l + k * N] = rm[l * d + k]; // column-major out
    if (cluster)
        for (i64 l = 0; l < N; l++) cluster[l] = lc[l] + 1;
    if (ledges || lw_e) { // rows in idx order / N*(i-1)+j order, w > 0 only (src/landmarks.jl:441-463)
        const i64 ne = c->n_ledges;
        i64 k = 0;
        for (i64 a = 0; a < N; a++)
            for (i64 b = c->lm_directed ? 0 : a; b < N; b++) {
                const double wv = we[a * N + b];
                if (wv > 0) {
                    if (k >= ne) CGE_THROW(CGE_E_ASSERT, "landmark edge count changed between run and fetch");
                    if (ledges) { ledges[k] = a + 1; ledges[k + ne] = b + 1; }
                    if (lw_e) lw_e[k] = wv;
                    k++;
                }
            }
    }
    if (v_to_l) { // 1-based landmark of every vertex (:379), from the device copy the score path works on
        std::vector<i32> v0(n);
        HIP_CHECK(hipMemcpyAsync(v0.data(), c->v2l.p, sizeof(i32) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        for (i64 i = 0; i < n; i++) v_to_l[i] = (i64)v0[i] + 1;
    }
}

// ---- samples of the local score -----------------------------------------------------------------------------------------------
// whether make_samples can be started ahead of the rest of a score: one seeded set, drawn on the device from a local edge list
static bool samples_can_start_early(cge_ctx *c, i64 seed, bool exact_directed) {
    return seed != -1 && !exact_directed && sampler_uses_device(c) && !c->edges_sharded;
}
// begin_only (samples_can_start_early): the draws and the first rejection round are enqueued, no synchronisation;
// k_draw_samples_finish does the rest
static void make_samples(cge_ctx *c, i64 seed, i64 S, int directed, bool exact_directed, SampleSet &smp, bool begin_only = false) {
    // seeded: one set reused at every alpha (Random.seed! before each draw, src/divergence.jl:184,193);
    // unseeded: a fresh set per alpha, keyed by an arbitrary fixed base seed and the alpha index
    smp.S = S;
    smp.n_sets = (seed != -1) ? 1 : AlphaBook::n_alpha;
    const i64 base = (seed != -1) ? seed : 0x5eedc0de;
    if (sampler_uses_device(c)) { // large resident graph: drawn, rejected and kept on the device (the same stream of draws)
        smp.on_device = true;
        smp.d_pos.ensure(smp.n_sets * S); smp.d_ni.ensure(smp.n_sets * S); smp.d_nj.ensure(smp.n_sets * S);
        if (begin_only) { // (one set, no second draw)
            k_draw_samples_begin(c, base, 0, S, directed, smp.d_pos.p, smp.d_ni.p, smp.d_nj.p);
            return;
        }
        for (i64 t = 0; t < smp.n_sets; t++)
            k_draw_samples_dev(c, base, t, S, directed, smp.d_pos.p + t * S, smp.d_ni.p + t * S, smp.d_nj.p + t * S);
        if (exact_directed) { // the un-reseeded second positive draw of :510 (its non-edges are not used)
            smp.d_pos2.ensure(smp.n_sets * S);
            DevBuf<i32> di, dj;
            di.ensure(S); dj.ensure(S);
            for (i64 t = 0; t < smp.n_sets; t++)
                k_draw_samples_dev(c, base + 0x7777, 1000 + t, S, directed, smp.d_pos2.p + t * S, di.p, dj.p);
        }
        return;
    }
    smp.pos_idx.resize(smp.n_sets * S);
    smp.neg_i.resize(smp.n_sets * S);
    smp.neg_j.resize(smp.n_sets * S);
    for (i64 t = 0; t < smp.n_sets; t++)
        host_draw_samples(c, base, t, S, directed, &smp.pos_idx[t * S], &smp.neg_i[t * S], &smp.neg_j[t * S]);
    if (exact_directed) { // the un-reseeded second positive draw of :510
        smp.pos_idx2.resize(smp.n_sets * S);
        std::vector<i64> di(S), dj(S);
        for (i64 t = 0; t < smp.n_sets; t++)
            host_draw_samples(c, base + 0x7777, 1000 + t, S, directed, &smp.pos_idx2[t * S], di.data(), dj.data());
    }
}

// ---- what cge_score and cge_wgcl share ----------------------------------------------------------------------------------------
static ScoreGraph score_graph(i64 N, i64 d, i64 C, const double *emb, const double *dist, const double *vw, const i32 *comm,
                              const double *vectC) {
    ScoreGraph G;
    G.N = N; G.d = d; G.C = C;
    G.emb = emb; G.dist = dist; G.vw = vw; G.comm = comm; G.vectC = vectC;
    return G;
}

// the directed degree pass of a score graph given as an edge list: in- / out-degrees (c->s_degin / s_degout) and star counts
// (common.hpp: the testing hook cge_sweep_setup_test calls it too)
void edge_degrees(cge_ctx *c, const i32 *src, const i32 *dst, const double *w, i64 m, i64 N, DevBuf<i32> &star) {
    hipStream_t st = c->stream;
    c->s_degin.ensure(N); c->s_degout.ensure(N); star.ensure(N);
    HIP_CHECK(hipMemsetAsync(c->s_degin.p, 0, sizeof(double) * N, st));
    HIP_CHECK(hipMemsetAsync(c->s_degout.p, 0, sizeof(double) * N, st));
    HIP_CHECK(hipMemsetAsync(star.p, 0, sizeof(i32) * N, st));
    k_edge_degrees(c, src, dst, w, m, c->s_degout.p, c->s_degin.p, star.p);
}

// star-graph guard of wGCL_directed (src/divergence.jl:321-334): the star counts of the degree pass are read back; a star graph
// gets the reference's 6-element return (true)
static bool star_return(cge_ctx *c, const i32 *d_star, i64 N, double out[7], int *out_len) {
    std::vector<i32> star(N);
    HIP_CHECK(hipMemcpyAsync(star.data(), d_star, sizeof(i32) * N, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    bool has_nm1 = false, has_2nm1 = false;
    i64 sum = 0, cnt2 = 0;
    for (i64 i = 0; i < N; i++) {
        if (star[i] == N - 1) has_nm1 = true;
        if (star[i] == 2 * (N - 1)) has_2nm1 = true;
        sum += star[i];
        if (star[i] == 2) cnt2++;
    }
    if (!((has_nm1 && sum == 2 * (N - 1)) || (has_2nm1 && cnt2 == N - 1))) return false;
    out[0] = -1.0;
    for (int k = 1; k < 6; k++) out[k] = 0.0;
    *out_len = 6;
    return true;
}
// what follows whichever degree pass applied: true = a star graph, `out` is written and the score is over; else the degrees
// (c->s_degin / s_degout) become the score graph's
static bool directed_guard(cge_ctx *c, ScoreGraph &G, const DevBuf<i32> &star, double out[7], int *out_len) {
    if (star_return(c, star.p, G.N, out, out_len)) return true;
    G.deg_in = c->s_degin.p;
    G.deg_out = c->s_degout.p;
    return false;
}

// what a landmark-mode sweep reads of the original graph: the resident one, with `lweight` as the landmarks' weights
static OrigView resident_orig_view(cge_ctx *c, const double *lweight) {
    OrigView ov;
    ov.n = c->n; ov.m = c->m; ov.Xr = c->Xr.p; ov.vw = c->vw.p; ov.v2l = c->v2l.p; ov.lweight = lweight;
    ov.src = c->src.p; ov.dst = c->dst.p; ov.h_w = c->h_w.empty() ? nullptr : c->h_w.data();
    return ov;
}

// the alpha sweep of a score graph; the local score samples the resident graph (`ov`: landmark mode)
static void sweep_resident(cge_ctx *c, const ScoreGraph &G, const OrigView *ov, int directed, int split, const SampleSet &smp,
                           double out[7], int *out_len, cge_trace *trace, SweepHandoff *defer = nullptr) {
    host_wgcl_sweep(c, G, ov, c->src.p, c->dst.p, c->h_w.empty() ? nullptr : c->h_w.data(), c->m, directed, split, smp, out, out_len,
                    trace, defer);
}

// ---- cge_score ----------------------------------------------------------------------------------------------------------------
struct Score {
    bool landmarks, reuse_samples; // reuse_samples (cge_score_batch): the local score's samples of this graph and seed are in c->smp
    // samples_early: the draw and the first round of the rejection are enqueued behind the first synchronisation of the landmark
    // phase, whose host-side set-up then leaves the device idle for a few hundred microseconds (score_samples looks at the verdict)
    bool samples_early;
    ScoreGraph G;
    OrigView ov;
    std::vector<i32> lcomm_host;
};

// the landmark graph as the score graph; directed: its degrees / star counts (c->s_star) from the landmark-pair matrix
static void score_graph_landmarks(cge_ctx *c, const cge_score_args *a, Score &S) {
    LandmarkRun R = score_landmark_run(c, a);
    lm_clamp(c, R);
    if (S.samples_early) { // (the host now sets up runsplit for a few hundred microseconds)
        c->smp.reset();
        make_samples(c, a->seed, a->auc_samples, a->directed, false, c->smp, true);
    }
    lm_split(c, R);
    lm_aggregate(c, R);
    lm_scatter(c, R);
    const i64 N = c->N;
    // wGCL's own `maximum(edges)` / size asserts (src/divergence.jl:41,50): the highest-numbered
    // landmark must carry an edge -- always true when every vertex has positive weight
    S.G = score_graph(N, c->d, c->n_comm_max, c->lemb.p, c->dii.p, c->lweight.p, c->lcomm.p, c->vectC.p);
    if (!a->directed) return;
    c->s_degin.ensure(N); c->s_degout.ensure(N); c->s_star.ensure(N);
    if (c->wedges_block_only) { // a reduce-scattered matrix: this rank's row block, then the ranks add the three vectors
        const RowBlock blk = wedge_row_block(c, N);
        DevBuf<double> &X = c->samp_xchg;
        X.ensure(3 * N);
        k_wedge_degrees_block(c, c->wedges.p, N, blk.r0, blk.r1, X.p);
        cge_allreduce_dev(c, X.p, 3 * N, 0);
        k_degrees_unpack(c, X.p, N, c->s_degout.p, c->s_degin.p, c->s_star.p);
    } else
        k_wedge_degrees(c, c->wedges.p, N, c->s_degout.p, c->s_degin.p, c->s_star.p);
}

// what the sweep of a landmark graph reads of the resident one, the diameter among it
static void score_landmark_view(cge_ctx *c, Score &S) {
    const double t0 = now_ms();
    const i64 N = c->N;
    S.ov = resident_orig_view(c, c->lweight.p);
    S.lcomm_host.resize(N); // community of a landmark = community of any member (landmarks never span two): :427
    HIP_CHECK(hipMemcpyAsync(S.lcomm_host.data(), c->lcomm.p, sizeof(i32) * N, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    S.ov.hi = host_diameter_landmarks(c, c->lemb.p, c->lweight.p, S.lcomm_host, c->n_comm_max, N);
    S.ov.h_lcomm = S.lcomm_host.data(); // (the sweep groups the landmarks by community: no second read-back)
    c->phases.ms["diameter"] = now_ms() - t0; // what the main thread still waited for
}

// exact mode: the resident graph itself as the score graph; directed: its degrees / star counts (c->s_star) from its edges
static void score_graph_exact(cge_ctx *c, const cge_score_args *a, Score &S) {
    if (c->edges_sharded)
        CGE_THROW(CGE_E_ARG, "score: exact mode reads the whole edge list on every rank; the resident one is sharded (option shard_ingest)");
    if (c->rows_sharded)
        CGE_THROW(CGE_E_ARG, "score: exact mode reads every embedding row on every rank; the resident rows are sharded (option shard_rows)");
    const i64 N = c->n, C = c->n_comm_max;
    DevBuf<double> &zeros = c->sw_zeros;
    zeros.ensure(N);
    HIP_CHECK(hipMemsetAsync(zeros.p, 0, sizeof(double) * N, c->stream)); // distances = zeros (CGE_CLI.jl:4)
    c->vectC.ensure(a->directed ? C * C : packed_len(C));
    scatter_vectC_resident(c, C, a->directed, c->vectC.p);
    S.G = score_graph(N, c->d, C, c->Xr.p, zeros.p, c->vw.p, c->comm.p, c->vectC.p);
    if (a->directed) edge_degrees(c, c->src.p, c->dst.p, c->unit_weights ? nullptr : c->w.p, c->m, N, c->s_star);
}

static void score_samples(cge_ctx *c, const cge_score_args *a, const Score &S) {
    const double t0 = now_ms();
    if (S.reuse_samples) { // (drawn for the first member; they depend on the graph and the seed only)
    } else if (S.samples_early && c->samp_pending.on) k_draw_samples_finish(c);
    else {
        c->smp.reset();
        make_samples(c, a->seed, a->auc_samples, a->directed, a->directed && !S.landmarks, c->smp);
    }
    c->phases.ms["samples"] = now_ms() - t0;
}

// cge_score's work on the resident inputs.  `defer` (cge_score_batch): a sweep on the fused path is prepared and handed over
// instead of run (host_wgcl_sweep).
void host_score(cge_ctx *c, const cge_score_args *a, double out[7], int *out_len, cge_trace *trace, SweepHandoff *defer,
                bool reuse_samples) {
    check_resident(c, "score");
    c->phases.ms.clear();
    Score S{a->land != -1, reuse_samples};
    S.samples_early = S.landmarks && !reuse_samples && samples_can_start_early(c, a->seed, false);
    // Whatever happens, an early draw does not outlive the call: a star graph's early return or an error in between leaves it
    // pending, and it is drained here (a score that got through has looked at its draw: no synchronisation then)
    struct DrainDraw {
        cge_ctx *c;
        ~DrainDraw() {
            if (c->samp_pending.on) (void)hipStreamSynchronize(c->stream);
            c->samp_pending.on = false;
        }
    } drain{c};
    if (S.landmarks) score_graph_landmarks(c, a, S);
    else score_graph_exact(c, a, S);
    if (a->directed && directed_guard(c, S.G, c->s_star, out, out_len)) return;
    if (S.landmarks) score_landmark_view(c, S);
    score_samples(c, a, S);
    const double t0 = now_ms();
    sweep_resident(c, S.G, S.landmarks ? &S.ov : nullptr, a->directed, a->split, c->smp, out, out_len, trace, defer);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->phases.ms[defer && defer->deferred ? "sweep_setup" : "sweep"] = now_ms() - t0;
    flush_timers(c);
}

// ---- cge_wgcl: everything as host arrays --------------------------------------------------------------------------------------
static void upload_i64_as_i32(cge_ctx *c, const i64 *h, i64 cnt, i64 lo, i64 hi, DevBuf<i32> &out, const char *what) {
    std::vector<i32> t(cnt);
    for (i64 i = 0; i < cnt; i++) {
        if (h[i] < lo || h[i] > hi) CGE_THROW(CGE_E_ARG, "%s: id %lld outside %lld..%lld", what, (long long)h[i], (long long)lo, (long long)hi);
        t[i] = (i32)(h[i] - 1);
    }
    out.ensure(cnt);
    HIP_CHECK(hipMemcpyAsync(out.p, t.data(), sizeof(i32) * cnt, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// landmark -> members CSR from a 0-based assignment: the members are this rank's rows (all vertices, or under option shard_rows
// its local row ids), ascending; sharded, the global sizes are kept too and the index goes to the device
static void build_landmark_index(cge_ctx *c, const std::vector<i32> &v2l0, i64 N) {
    const bool sharded = c->rows_sharded;
    const i64 n = (i64)v2l0.size(), nl = sharded ? c->n_loc : n;
    auto landmark_of = [&](i64 i) { return v2l0[sharded ? c->h_loc2glob[i] : i]; };
    c->h_mem_off.assign(N + 1, 0);
    c->h_mem.resize(nl);
    for (i64 i = 0; i < nl; i++) c->h_mem_off[landmark_of(i) + 1]++;
    for (i64 l = 0; l < N; l++) c->h_mem_off[l + 1] += c->h_mem_off[l];
    std::vector<i32> cur(c->h_mem_off.begin(), c->h_mem_off.end() - 1);
    for (i64 i = 0; i < nl; i++) c->h_mem[cur[landmark_of(i)]++] = (i32)i;
    c->lm_index_on_device = sharded;
    if (!sharded) return;
    c->h_gl_off.assign(N + 1, 0);
    for (i64 i = 0; i < n; i++) c->h_gl_off[v2l0[i] + 1]++;
    for (i64 l = 0; l < N; l++) c->h_gl_off[l + 1] += c->h_gl_off[l];
    c->lm_memoff.ensure(N + 1);
    c->lm_mem.ensure(nl);
    HIP_CHECK(hipMemcpyAsync(c->lm_memoff.p, c->h_mem_off.data(), sizeof(i32) * (N + 1), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(c->lm_mem.p, c->h_mem.data(), sizeof(i32) * nl, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

struct Wgcl {
    i64 N = 0, C = 0; // vertices and communities of the score graph
    bool landmarks = false;
    DevBuf<i32> g_src, g_dst, star; // the score graph's edges and star counts, the caller's embedding: device scratch of this call
    DevBuf<double> g_w, colbuf;
    ScoreGraph G;
    OrigView ov;
    SampleSet smp;
};

static void wgcl_check(const cge_wgcl_args *a, Wgcl &S) {
    if (!a->edges_src || !a->edges_dst || a->m <= 0) CGE_THROW(CGE_E_ARG, "wGCL: empty edge list");
    i64 N = 0;
    for (i64 e = 0; e < a->m; e++) N = std::max(N, std::max(a->edges_src[e], a->edges_dst[e])); // maximum(edges) :41
    S.landmarks = a->n_v_to_l > 0;                                                                // :44
    if (a->n_comm != N) CGE_THROW(CGE_E_ASSERT, "AssertionError: No. communities not matching no. vertices"); // :50
    if (a->n_distances != N) CGE_THROW(CGE_E_ASSERT, "AssertionError: Distances vector length is not equal to no. vertices"); // :81
    if (a->embed_rows < N) CGE_THROW(CGE_E_ARG, "wGCL: embedding has fewer rows than vertices");
    S.N = N;
    for (i64 i = 0; i < N; i++) S.C = std::max(S.C, a->comm[i]);
}

// score graph -> device scratch; directed: its degrees / star counts from its edges
static void wgcl_upload_score_graph(cge_ctx *c, const cge_wgcl_args *a, Wgcl &S) {
    const i64 N = S.N, C = S.C, d = a->d;
    hipStream_t st = c->stream;
    upload_i64_as_i32(c, a->edges_src, a->m, 1, N, S.g_src, "edges");
    upload_i64_as_i32(c, a->edges_dst, a->m, 1, N, S.g_dst, "edges");
    S.g_w.ensure(a->m);
    HIP_CHECK(hipMemcpyAsync(S.g_w.p, a->eweights, sizeof(double) * a->m, hipMemcpyHostToDevice, st));
    upload_i64_as_i32(c, a->comm, N, 1, C, c->s_comm, "comm");
    S.colbuf.ensure((size_t)a->embed_rows * d);
    HIP_CHECK(hipMemcpyAsync(S.colbuf.p, a->embed, sizeof(double) * a->embed_rows * d, hipMemcpyHostToDevice, st));
    c->s_emb.ensure((size_t)a->embed_rows * d);
    k_transpose_to_rowmajor(c, S.colbuf.p, c->s_emb.p, a->embed_rows, d);
    c->s_dist.ensure(N);
    c->s_vw.ensure(N);
    HIP_CHECK(hipMemcpyAsync(c->s_dist.p, a->distances, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->s_vw.p, a->vweights, sizeof(double) * N, hipMemcpyHostToDevice, st));
    const i64 vlen = a->directed ? C * C : packed_len(C);
    c->s_vectC.ensure(vlen);
    HIP_CHECK(hipMemsetAsync(c->s_vectC.p, 0, sizeof(double) * vlen, st));
    k_edge_scatter(c, S.g_src.p, S.g_dst.p, S.g_w.p, 0, a->m, nullptr, c->s_comm.p, N, C, a->directed, nullptr, c->s_vectC.p);
    S.G = score_graph(N, d, C, c->s_emb.p, c->s_dist.p, c->s_vw.p, c->s_comm.p, c->s_vectC.p);
    if (a->directed) edge_degrees(c, S.g_src.p, S.g_dst.p, S.g_w.p, a->m, N, S.star);
    HIP_CHECK(hipStreamSynchronize(st));
}

// the graph the local score samples from: the original graph in landmark mode (the init_* arrays made resident, or what is
// resident already), else the score graph, made resident so that the sampler can reject its edges
static void wgcl_original_graph(cge_ctx *c, const cge_wgcl_args *a, Wgcl &S) {
    const i64 N = S.N;
    if (!S.landmarks) {
        set_graph(c, a->edges_src, a->edges_dst, a->eweights, a->m, N);
        return;
    }
    if (a->init_embed && a->init_edges_src && a->init_edges_dst && a->init_vweights) {
        const i64 n0 = a->n_init;
        if (a->n_v_to_l != n0) CGE_THROW(CGE_E_ARG, "wGCL: v_to_l and init_vweights differ in length");
        const cge_embedding_view emb = {a->init_embed, a->d, 0, CGE_DTYPE_F64, 0, 0};
        set_graph(c, a->init_edges_src, a->init_edges_dst, a->init_eweights, a->m_init, n0);
        if (a->d <= 0) throw CgeError{CGE_E_ARG, c->err}; // (cge_set_embedding's bare status: the message stays)
        set_embedding_view(c, "set_embedding", &emb, n0);
        set_vertex_data(c, nullptr, a->init_vweights, n0);
    } else if (!c->Xr.p || !c->src.p || !c->vw.p || c->n != a->n_v_to_l)
        CGE_THROW(CGE_E_ARG, "wGCL: landmark mode needs init_* arrays or matching resident inputs");
    upload_i64_as_i32(c, a->v_to_l, a->n_v_to_l, 1, N, c->v2l, "v_to_l");
    std::vector<i32> v2l0(a->n_v_to_l), lcomm0(N);
    for (i64 i = 0; i < a->n_v_to_l; i++) v2l0[i] = (i32)(a->v_to_l[i] - 1);
    build_landmark_index(c, v2l0, N);
    S.ov = resident_orig_view(c, c->s_vw.p);
    for (i64 i = 0; i < N; i++) lcomm0[i] = (i32)(a->comm[i] - 1);
    S.ov.hi = host_diameter_landmarks(c, c->s_emb.p, c->s_vw.p, lcomm0, S.C, N);
}

// the caller's draws, or the library's
static void wgcl_samples(cge_ctx *c, const cge_wgcl_args *a, Wgcl &S) {
    SampleSet &smp = S.smp;
    if (!(a->pos_idx && a->neg_i && a->neg_j && a->n_sample_sets > 0)) {
        make_samples(c, a->seed, a->auc_samples, a->directed, a->directed && !S.landmarks, smp);
        return;
    }
    if (c->edges_sharded) CGE_THROW(CGE_E_ARG, "wGCL: caller-drawn samples index the whole edge list, the resident one is sharded (option shard_ingest)");
    smp.S = a->auc_samples;
    smp.n_sets = a->n_sample_sets;
    const i64 tot = smp.S * smp.n_sets;
    smp.pos_idx.assign(a->pos_idx, a->pos_idx + tot);
    smp.neg_i.assign(a->neg_i, a->neg_i + tot);
    smp.neg_j.assign(a->neg_j, a->neg_j + tot);
    if (a->pos_idx2) smp.pos_idx2.assign(a->pos_idx2, a->pos_idx2 + tot);
}

void host_wgcl(cge_ctx *c, const cge_wgcl_args *a, double out[7], int *out_len, cge_trace *trace) {
    // the score graph of this entry point (and the init_* graph it may upload) is held whole on every rank
    struct KeepOption { int &ref; int val; ~KeepOption() { ref = val; } } keep_ingest{c->opt_shard_ingest, c->opt_shard_ingest};
    c->opt_shard_ingest = 0;
    Wgcl S;
    wgcl_check(a, S);
    wgcl_upload_score_graph(c, a, S);
    if (a->directed && directed_guard(c, S.G, S.star, out, out_len)) return;
    wgcl_original_graph(c, a, S);
    wgcl_samples(c, a, S);
    sweep_resident(c, S.G, S.landmarks ? &S.ov : nullptr, a->directed, a->split, S.smp, out, out_len, trace);
    flush_timers(c);
}

// ---- single passes the boundary offers on their own ---------------------------------------------------------------------------
// vI (when given) selects bins; the device kernel derives the diagonal mask from the packed/square layout, so here the selected
// bins are compacted on the host first and scored with mode 0.
void host_js(cge_ctx *c, const double *vC, const double *vB, i64 len, const uint8_t *vI, int internal, double *out) {
    std::vector<double> p, q;
    for (i64 k = 0; k < len; k++)
        if (!vI || ((vI[k] != 0) == (internal != 0))) { p.push_back(vC[k]); q.push_back(vB[k]); }
    const i64 L = (i64)p.size();
    DevBuf<double> dp, dq, r;
    dp.ensure(L); dq.ensure(L); r.ensure(1);
    HIP_CHECK(hipMemcpyAsync(dp.p, p.data(), sizeof(double) * L, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(dq.p, q.data(), sizeof(double) * L, hipMemcpyHostToDevice, c->stream));
    k_js(c, dp.p, dq.p, L, 1, 0, 0, r.p);
    HIP_CHECK(hipMemcpyAsync(out, r.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

void host_edge_scatter(cge_ctx *c, const int64_t *v_to_l, i64 N, i64 C, int directed, i64 e0, i64 e1, double *wedges_out,
                       double *vect_C_out) {
    if (!c->src.p || !c->comm.p) CGE_THROW(CGE_E_ARG, "edge_scatter: graph and vertex data must be resident");
    if (c->edges_sharded) CGE_THROW(CGE_E_ARG, "edge_scatter: the resident edge list is sharded over the ranks (option shard_ingest)");
    if (e1 > c->m) CGE_THROW(CGE_E_ARG, "edge_scatter: edge range beyond m");
    hipStream_t st = c->stream;
    DevBuf<i32> dv;
    if (v_to_l) upload_i64_as_i32(c, v_to_l, c->n, 1, N, dv, "v_to_l");
    const i64 vlen = directed ? C * C : packed_len(C);
    DevBuf<double> dw, dc;
    if (wedges_out) {
        if (!v_to_l) CGE_THROW(CGE_E_ARG, "edge_scatter: wedges need v_to_l");
        dw.ensure((size_t)N * N);
        HIP_CHECK(hipMemsetAsync(dw.p, 0, sizeof(double) * N * N, st));
    }
    if (vect_C_out) {
        dc.ensure(vlen);
        HIP_CHECK(hipMemsetAsync(dc.p, 0, sizeof(double) * vlen, st));
    }
    if (!wedges_out && vect_C_out && e0 == 0 && e1 == c->m && C == c->n_comm_max && !c->has_coll)
        scatter_vectC_resident(c, C, directed, dc.p); // the score path's forms of the whole-list pass
    else
        k_edge_scatter(c, c->src.p, c->dst.p, c->unit_weights ? nullptr : c->w.p, e0, e1, v_to_l ? dv.p : nullptr,
                       c->comm.p, N, C, directed, wedges_out ? dw.p : nullptr, vect_C_out ? dc.p : nullptr);
    if (wedges_out) HIP_CHECK(hipMemcpyAsync(wedges_out, dw.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
    if (vect_C_out) HIP_CHECK(hipMemcpyAsync(vect_C_out, dc.p, sizeof(double) * vlen, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    flush_timers(c);
}

// Testing hook (include/cge_hip_testing.h: cge_landmark_graph_test): the stage between the split and the score graph on a
// caller's assignment -- build_landmark_index + aggregate_landmarks, scatter_wedges_share with the one-rank count behind it, and
// the degree kernels of the directed score, each as lm_aggregate, scatter_wedges and score_graph_landmarks call them.  The
// shares and row blocks of pretend ranks come from EdgeShare and row_block_of.
void host_landmark_graph_test(cge_ctx *c, cge_landmark_graph_io *io) {
    const i64 N = io->N, n = c->n, d = c->d;
    hipStream_t st = c->stream;
    const bool want_agg = io->lemb || io->lweight || io->dii || io->lcomm;
    const bool want_deg = io->deg_out || io->deg_in || io->star;
    const bool want_blk = io->deg_block || io->u_deg_out || io->u_deg_in || io->u_star;
    const bool want_mat = io->wedges || io->positive || want_deg || want_blk;
    if (c->rows_sharded || c->edges_sharded)
        CGE_THROW(CGE_E_ARG, "landmark_graph_test: not with option shard_rows / shard_ingest (every row and edge on one rank)");
    if (n <= 0) CGE_THROW(CGE_E_ARG, "landmark_graph_test: nothing is resident");
    if (want_mat && (!c->src.p || !c->dst.p || c->m <= 0 || (!c->unit_weights && !c->w.p)))
        CGE_THROW(CGE_E_ARG, "landmark_graph_test: the graph is not resident (cge_set_graph)");
    if (want_agg && (!c->Xr.p || d <= 0 || c->Xr.n < (size_t)(n * d) || !c->vw.p || !c->comm.p || c->vw.n < (size_t)n || c->comm.n < (size_t)n))
        CGE_THROW(CGE_E_ARG, "landmark_graph_test: the aggregate needs the embedding and the vertex data resident");
    if (io->nparts < 1 || io->part < 0 || io->part >= io->nparts) CGE_THROW(CGE_E_ARG, "landmark_graph_test: part %lld of %lld", (long long)io->part, (long long)io->nparts);
    if (want_blk && (io->world < 1 || io->world > 64)) CGE_THROW(CGE_E_ARG, "landmark_graph_test: world %lld outside 1..64", (long long)io->world);
    if (want_blk && (!io->deg_block || !io->u_deg_out || !io->u_deg_in || !io->u_star))
        CGE_THROW(CGE_E_ARG, "landmark_graph_test: the block form of the degrees returns deg_block and the three unpacked vectors together");
    if (want_mat && N > 46340) CGE_THROW(CGE_E_ARG, "landmark_graph_test: N = %lld, the matrix is beyond 2^31 entries", (long long)N);
    std::vector<i32> v2l0(n);
    for (i64 i = 0; i < n; i++) {
        if (io->v2l[i] < 1 || io->v2l[i] > N)
            CGE_THROW(CGE_E_ARG, "landmark_graph_test: v_to_l: id %lld outside 1..%lld", (long long)io->v2l[i], (long long)N);
        v2l0[i] = (i32)(io->v2l[i] - 1);
    }
    if (want_agg) {
        std::vector<char> seen(N, 0);
        for (i64 i = 0; i < n; i++) seen[v2l0[i]] = 1;
        for (i64 l = 0; l < N; l++)
            if (!seen[l]) CGE_THROW(CGE_E_ARG, "landmark_graph_test: landmark %lld has no member (the aggregate needs one)", (long long)(l + 1));
    }
    // the geometry of this share, before any launch
    const EdgeShare mine{io->part, io->nparts};
    WedgeGeometry G{};
    bool geom = false;
    io->n_chunks = 0;
    if (want_mat) {
        const bool blocked = c->blocked_ready || (k_blocked_edges_possible(c) && k_build_blocked_edges(c));
        io->n_chunks = blocked ? c->be_nchunks : 0;
        geom = blocked && k_wedge_geometry(N, c->unit_weights ? 4 : 8, std::max<i64>(mine.hi(c->be_nchunks) - mine.lo(c->be_nchunks), 1), &G);
        if (io->wedge_form == 1 && !geom)
            CGE_THROW(CGE_E_ARG, "landmark_graph_test: the tiled form declines N = %lld over %lld chunks (%s)", (long long)N,
                      (long long)io->n_chunks, blocked ? "its geometry" : "no blocked edge list");
    }
    // what a landmark run left behind is replaced
    c->lm_ready = false;
    c->wedges_ready = false;
    c->n_ledges = -1;
    c->h_v2l.clear();
    c->v2l.ensure(n);
    HIP_CHECK(hipMemcpyAsync(c->v2l.p, v2l0.data(), sizeof(i32) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    io->form_ran = 0;
    io->rshift = io->colbits = -1;
    io->ntile = -1;
    if (want_agg) {
        build_landmark_index(c, v2l0, N);
        c->lm_memoff.ensure(N + 1);
        c->lm_mem.ensure(n);
        HIP_CHECK(hipMemcpyAsync(c->lm_memoff.p, c->h_mem_off.data(), sizeof(i32) * (N + 1), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(c->lm_mem.p, c->h_mem.data(), sizeof(i32) * n, hipMemcpyHostToDevice, st));
        c->lm_index_on_device = true;
        aggregate_landmarks(c, N);
        if (io->lemb) HIP_CHECK(hipMemcpyAsync(io->lemb, c->lemb.p, sizeof(double) * N * d, hipMemcpyDeviceToHost, st));
        if (io->lweight) HIP_CHECK(hipMemcpyAsync(io->lweight, c->lweight.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        if (io->dii) HIP_CHECK(hipMemcpyAsync(io->dii, c->dii.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        if (io->lcomm) HIP_CHECK(hipMemcpyAsync(io->lcomm, c->lcomm.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (want_mat) {
        c->wedges.ensure((size_t)N * N);
        c->wedges_block_only = false;
        DevBuf<i64> &cnt = c->wed_cnt;
        cnt.ensure(1);
        const bool tiled = scatter_wedges_share(c, c->v2l.p, N, io->directed, mine, io->wedge_form, c->wedges.p, cnt.p);
        if (tiled != (io->wedge_form == 2 ? false : geom))
            CGE_THROW(CGE_E_ASSERT, "landmark_graph_test: the tiled form %s against its geometry's verdict", tiled ? "ran" : "declined");
        if (!tiled) k_compact_count(c, c->wedges.p, N, io->directed, cnt.p); // (one rank: scatter_wedges)
        io->form_ran = tiled ? 1 : 2;
        if (tiled) { io->rshift = G.rshift; io->colbits = G.colbits; io->ntile = G.ntile; }
        if (io->wedges) HIP_CHECK(hipMemcpyAsync(io->wedges, c->wedges.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
        if (io->positive) HIP_CHECK(hipMemcpyAsync(io->positive, cnt.p, sizeof(i64), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (want_deg || want_blk) { c->s_degin.ensure(N); c->s_degout.ensure(N); c->s_star.ensure(N); }
    if (want_deg) {
        k_wedge_degrees(c, c->wedges.p, N, c->s_degout.p, c->s_degin.p, c->s_star.p);
        if (io->deg_out) HIP_CHECK(hipMemcpyAsync(io->deg_out, c->s_degout.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        if (io->deg_in) HIP_CHECK(hipMemcpyAsync(io->deg_in, c->s_degin.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        if (io->star) HIP_CHECK(hipMemcpyAsync(io->star, c->s_star.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (want_blk) { // every pretend rank's row block, the ranks' sum (in rank order) on the host, then the unpack
        DevBuf<double> X;
        X.ensure(3 * N);
        std::vector<double> sum(3 * N, 0.0);
        for (i64 r = 0; r < io->world; r++) {
            const RowBlock blk = row_block_of(N, r, io->world);
            double *out = io->deg_block + r * 3 * N;
            k_wedge_degrees_block(c, c->wedges.p, N, blk.r0, blk.r1, X.p);
            HIP_CHECK(hipMemcpyAsync(out, X.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            for (i64 k = 0; k < 3 * N; k++) sum[k] += out[k];
        }
        HIP_CHECK(hipMemcpyAsync(X.p, sum.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice, st));
        k_degrees_unpack(c, X.p, N, c->s_degout.p, c->s_degin.p, c->s_star.p);
        HIP_CHECK(hipMemcpyAsync(io->u_deg_out, c->s_degout.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(io->u_deg_in, c->s_degin.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(io->u_star, c->s_star.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    flush_timers(c);
}
