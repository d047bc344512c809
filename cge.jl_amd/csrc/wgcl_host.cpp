// wgcl_host.cpp -- host side of the alpha sweep (wGCL / wGCL_directed, src/divergence.jl:27-257,
// :282-561) and the local-score sampler.  The host owns only the alpha bookkeeping (best/patience
// counters, :215-223, :242-253) and the batch-wise launch of fit iterations; every O(N^2) loop of the
// reference runs in kernels_fit.hip / kernels_dist.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "sweep_internal.hpp"

// the counter-based RNG of the sampler lives in common.hpp (the device draws the same stream)
static inline uint64_t ctr_rand(uint64_t seed, uint64_t stream, uint64_t k, uint64_t attempt, uint64_t which) {
    return cge_ctr_rand(seed, stream, k, attempt, which);
}
static inline uint64_t bounded(uint64_t r, uint64_t range) { return cge_bounded(r, range); }

void host_pos_draw(i64 seed, i64 stream_id, i64 S, i64 m, i64 *pos_idx) {
    for (i64 k = 0; k < S; k++)
        pos_idx[k] = (i64)bounded(ctr_rand((uint64_t)seed, (uint64_t)stream_id, (uint64_t)k, 0, 0), (uint64_t)m) + 1;
}

// `sample(E, S, replace=true)` and `sample(NE, S, replace=true)` (src/divergence.jl:185,194,203,210;
// directed :485,495,505,513) on the RESIDENT graph.  Uniform with replacement over the edge rows and
// over the non-edge pairs (rejection against the resident edge list, checked on the device).
void host_draw_samples(cge_ctx *c, i64 seed, i64 stream_id, i64 S, int directed, i64 *pos_idx, i64 *neg_i, i64 *neg_j) {
    const i64 n = c->n, m = c->m;
    if (m <= 0 || n < 2) CGE_THROW(CGE_E_ARG, "draw_samples: no resident graph");
    const uint64_t sd = (uint64_t)seed, st = (uint64_t)stream_id;
    host_pos_draw(seed, stream_id, S, m, pos_idx);
    // Small graphs (n(n-1) <= 2^25): enumerate NE itself (lexicographic order) and index into it --
    // exact and immune to dense graphs; larger graphs: rejection against the edge list.
    if ((double)n * (double)(n - 1) <= 33554432.0) {
        std::vector<i32> hs(m), hd(m);
        HIP_CHECK(hipMemcpyAsync(hs.data(), c->src.p, sizeof(i32) * m, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(hd.data(), c->dst.p, sizeof(i32) * m, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        std::vector<uint8_t> adj((size_t)n * n, 0);
        for (i64 e = 0; e < m; e++) {
            i64 a = hs[e], b = hd[e];
            if (!directed && a > b) std::swap(a, b);
            adj[(size_t)a * n + b] = 1;
        }
        std::vector<uint32_t> ne;
        ne.reserve((size_t)n * (n - 1) / (directed ? 1 : 2));
        for (i64 i = 0; i < n; i++)
            for (i64 j = directed ? 0 : i + 1; j < n; j++)
                if (i != j && !adj[(size_t)i * n + j]) ne.push_back((uint32_t)(i * n + j));
        if (ne.empty()) CGE_THROW(CGE_E_ARG, "draw_samples: the graph has no non-edges");
        for (i64 k = 0; k < S; k++) {
            const uint32_t code = ne[bounded(ctr_rand(sd, st, (uint64_t)k, 0, 1), (uint64_t)ne.size())];
            neg_i[k] = (i64)(code / n) + 1;
            neg_j[k] = (i64)(code % n) + 1;
        }
        return;
    }
    // large graphs: drawn and rejected against the resident edge list on the device (kernels_fit.hip), copied back here
    DevBuf<i32> d_pos, d_ni, d_nj;
    d_pos.ensure(S); d_ni.ensure(S); d_nj.ensure(S);
    k_draw_samples_dev(c, seed, stream_id, S, directed, d_pos.p, d_ni.p, d_nj.p);
    std::vector<i32> hi_(S), hj_(S);
    HIP_CHECK(hipMemcpyAsync(hi_.data(), d_ni.p, sizeof(i32) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(hj_.data(), d_nj.p, sizeof(i32) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    for (i64 k = 0; k < S; k++) {
        neg_i[k] = (i64)hi_[k] + 1;
        neg_j[k] = (i64)hj_[k] + 1;
    }
}
bool sampler_uses_device(const cge_ctx *c) { return (double)c->n * (double)(c->n - 1) > 33554432.0; }

// ------------------------------------------------------------------------------------------------

// Endpoints / weights of sampled edge rows are gathered on the host from small D2H reads of the
// resident edge arrays (S entries), so no host mirror of the edge list is needed.
static void gather_rows(cge_ctx *c, const i32 *d_arr, const std::vector<i64> &rows0, std::vector<i32> &out,
                        DevBuf<i32> &d_idx, DevBuf<i32> &d_out) {
    const i64 S = (i64)rows0.size();
    std::vector<i32> idx(S);
    for (i64 k = 0; k < S; k++) idx[k] = (i32)rows0[k];
    d_idx.ensure(S);
    d_out.ensure(S);
    out.resize(S);
    HIP_CHECK(hipMemcpyAsync(d_idx.p, idx.data(), sizeof(i32) * S, hipMemcpyHostToDevice, c->stream));
    k_gather_i32(c, d_arr, d_idx.p, S, d_out.p);
    HIP_CHECK(hipMemcpyAsync(out.data(), d_out.p, sizeof(i32) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// full_graph_D of sampled vertex pairs (src/divergence.jl:104-114 restricted to the draws), dist()'s own arithmetic.  Option
// shard_rows: a pair's two rows may live on two ranks -- the rows of a chunk of pairs are gathered from their owners into a
// zero-filled buffer (all-reduce of the words: exact) and every rank evaluates the chunk from the gathered rows.
void sampled_pair_dist(cge_ctx *c, const double *Xr, i64 d, const i32 *pi, const i32 *pj, i64 S, double den, double *out) {
    if (!c->rows_sharded) {
        k_pair_dist(c, Xr, d, pi, pj, S, den, out);
        return;
    }
    const i64 K = std::max<i64>(1024, std::min<i64>(S, ((i64)64 << 20) / (2 * d * 8))); // <= 64 MB of rows per exchange
    DevBuf<double> &B = c->samp_xchg;
    DevBuf<i32> &idx = c->epd_i;
    B.ensure((size_t)2 * K * d);
    idx.ensure(2 * K);
    for (i64 k0 = 0; k0 < S; k0 += K) {
        const i64 kc = std::min(K, S - k0);
        k_pair_local_idx(c, pi + k0, pj + k0, kc, c->glob2loc.p, idx.p);
        k_gather_rows_f64(c, c->Xr.p, c->n_loc, d, 1, idx.p, 2 * kc, B.p);
        cge_allreduce_dev(c, B.p, 2 * kc * d, 2);
        k_pair_dist_rows(c, B.p, d, pi + k0, pj + k0, kc, den, out + k0);
    }
}

// ---- the set-up of a sweep -------------------------------------------------------------------------

// The layout decision from the communities alone (hcomm: 0-based, on the host): the community CSR, the tile tables (on the
// device when the tiles apply), c->bvec_blocks / c->bvec_contig and, for a relabelled sweep, the order (lay.cm_mem) and its
// inverse on the device.  landmarks: a landmark-mode sweep.  force_relabel: the testing hook's contiguous-row form below 8193
// vertices (every sweep passes false).  Shared by plan_layout and the testing hook cge_vect_b_test.
// packed_req: the sweep wants the packed form of its matrix, which goes with the tile form of vect_B at any N >= 256.
void layout_tables(cge_ctx *c, const i32 *hcomm, i64 N, i64 C, int directed, bool landmarks, bool force_relabel,
                   SweepLayout &lay, bool packed_req) {
    std::vector<i32> &cm_off = lay.cm_off, &cm_mem = lay.cm_mem;
    // community -> members CSR of the score graph
    cm_off.assign(C + 1, 0);
    cm_mem.resize(N);
    for (i64 i = 0; i < N; i++) {
        if (hcomm[i] < 0 || hcomm[i] >= C) CGE_THROW(CGE_E_ARG, "community id out of range");
        cm_off[hcomm[i] + 1]++;
    }
    for (i64 q = 0; q < C; q++) cm_off[q + 1] += cm_off[q];
    {
        std::vector<i32> cur(cm_off.begin(), cm_off.end() - 1);
        for (i64 i = 0; i < N; i++) cm_mem[cur[hcomm[i]]++] = (i32)i;
    }
    // Exact mode beyond the LDS-staged vect_B (N > 8192): the score graph is RELABELLED so that every community is a range
    // of consecutive vertices (members keep their ascending order, so every community sum adds in the reference's order).
    // vect_B then reads its members as contiguous runs of a row -- with the vertex ids of a real graph (no relation to
    // the communities) it was a 8-byte gather per element, 93 ms per alpha at n = 60 000 against 3 ms for the stream.
    // Only what is indexed by vertex moves: embedding rows, weights / degrees, communities, the sampled pairs.
    // (also the landmark graph of a landmark-mode score with more than 8192 landmarks -- config 5 has 12 000; the local
    // score then reads T through the landmark ids of the original numbering, see the un-permuted copy in the sweep)
    // Option bvec_blocks = 1: an exact-mode sweep is relabelled from 256 vertices on and vect_B is summed BY TILES (kernels_fit.hip:
    // bvec_tile_kernel + bins: GD read once, no row bins) instead of row bins + row sums + fold (the same speed there,
    // profiles/r04_bvec_tiles_ab.txt); landmark-mode sweeps always do (below).
    // (beyond 8192 vertices the sweep is relabelled anyway and the staged row-bin kernel no longer fits LDS: there the tile
    // form replaces the plain gather -- config 5, N = 12 000: 1.1 ms per alpha for the row bins alone)
    const bool blocks_req = (c->opt_bvec_blocks || N > 8192 || packed_req) && c->opt_exact_relabel && N >= 256 && C >= 2 &&
                            !c->opt_test_bvec_plain;
    // Round 5, the default in landmark mode wherever the undirected persistent fit runs with one tile per wave: the rest of
    // an alpha's chain RIDES ON THE FIT'S LAUNCH (kernels_fitp.hip, fit_flow_kernel<.., true>: the power matrix in its
    // prologue, vect_B's tile partials and the local score's tallies in its epilogue).  It needs the relabelled sweep and the
    // tile tables below; option "fit_fused" = 0 keeps the separate launches (the cross-check of the parity tests).
    // Every undirected landmark-mode sweep of >= 256 landmarks is relabelled and sums vect_B by tiles then, whichever form of the
    // fit runs (so that all forms add in the same order and give the same bits); the fused launch itself needs the default
    // persistent form with one tile per wave.
    const bool tiles_req = landmarks && !directed && c->opt_fit_fused && c->opt_exact_relabel && N >= 256 &&
                           C >= 2 && !c->opt_test_bvec_plain;
    const bool fuse_req = tiles_req && !c->fit_persistent_broken && c->opt_fit_persistent != 1 &&
                          c->opt_pow_exp2 && flow_fused_applies(c, N);
    const bool blocks = blocks_req || tiles_req;
    bool blocks_ok = blocks, pieces_ok = true;
    // the sweep's small tables travel together: one pinned staging buffer, one copy and one scatter kernel per flush instead of a
    // copy from pageable memory (~20 us of idle stream) per table and a synchronisation wherever a table is a local
    WordPacker pk(c);
    std::vector<i32> bt_fc, bt_ns, bt_base;
    if (blocks) { // per 64-vertex block of the relabelled graph: first community and number of communities; per tile: its partials
        const i64 Nt = (N + 63) / 64;
        std::vector<i32> comm_new(N);
        for (i64 q2 = 0; q2 < C; q2++)
            for (i32 t2 = cm_off[q2]; t2 < cm_off[q2 + 1]; t2++) comm_new[t2] = (i32)q2; // position t2 of the community-sorted order
        bt_fc.resize(Nt); bt_ns.resize(Nt); bt_base.assign(Nt * Nt + 1, 0);
        for (i64 b = 0; b < Nt; b++) {
            bt_fc[b] = comm_new[64 * b];
            bt_ns[b] = comm_new[std::min<i64>(N, 64 * b + 64) - 1] - bt_fc[b] + 1;
            if (bt_ns[b] > 64) blocks_ok = false; // (empty communities in between: the row-bin form takes such a graph)
            // the fused epilogue stages one "piece" per run of a community inside an 8-column chunk (the tail beyond N is a run)
            int pieces = 0;
            for (i64 q = 0; q < 64; q++) {
                const i64 v = 64 * b + q, u = v - 1;
                const i32 cv = v < N ? comm_new[v] : -1, cu = (q > 0) ? (u < N ? comm_new[u] : -1) : -2;
                if ((q & 7) == 0 || cv != cu) pieces++;
            }
            if (pieces > CGE_FLOW_NP) pieces_ok = false;
        }
        i64 tot = 0;
        for (i64 I = 0; I < Nt && blocks_ok; I++)
            for (i64 J = 0; J < Nt; J++) {
                bt_base[I * Nt + J] = (i32)tot;
                if (directed || J >= I) tot += (i64)bt_ns[I] * bt_ns[J];
                if (tot > (i64)1 << 30) blocks_ok = false;
            }
        lay.bt_total = tot;
        if (blocks_ok) {
            c->sw_bt_fc.ensure(Nt); c->sw_bt_ns.ensure(Nt); c->sw_bt_base.ensure(Nt * Nt + 1); c->sw_bt_part.ensure(std::max<i64>(tot, 1) + 1); // (+ the +0.0 slot of k_bins_prepare)
            pk.add(c->sw_bt_fc.p, bt_fc.data(), Nt);
            pk.add(c->sw_bt_ns.p, bt_ns.data(), Nt);
            pk.add(c->sw_bt_base.p, bt_base.data(), Nt * Nt);
        }
    }
    lay.fuse = fuse_req && blocks_ok && pieces_ok;
    if (!blocks_req && !tiles_req) blocks_ok = false;
    lay.relabel = (N > 8192 && c->opt_exact_relabel) || blocks_ok || force_relabel;
    c->bvec_blocks = blocks_ok;
    c->bvec_contig = lay.relabel && N >= 64 * C; // a wave per (row, community) pays off for communities of a wave's width or more
    if (!lay.relabel) return;
    DevBuf<i32> &d_order = c->sw_rl_order;
    d_order.ensure(N);
    lay.old2new.ensure(N);
    std::vector<i32> old2new(N);
    for (i64 q = 0; q < N; q++) old2new[cm_mem[q]] = (i32)q;
    pk.add(d_order.p, cm_mem.data(), N);
    pk.add(lay.old2new.p, old2new.data(), N);
    pk.flush(); // (with the tile tables above)
}

// The layout decision, the tile tables and the relabelled copies of the score graph's per-vertex arrays (G points at them then).
// force_relabel: layout_tables' (the testing hook cge_sweep_setup_test; every sweep passes false).
void plan_layout(cge_ctx *c, ScoreGraph &G, const OrigView *orig, int directed, SweepLayout &lay, bool packed_req,
                 bool force_relabel) {
    const i64 N = G.N, d = G.d;
    std::vector<i32> hcomm(N);
    if (orig && orig->h_lcomm) std::memcpy(hcomm.data(), orig->h_lcomm, sizeof(i32) * N); // (the caller read them back for the diameter)
    else {
        HIP_CHECK(hipMemcpyAsync(hcomm.data(), G.comm, sizeof(i32) * N, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    layout_tables(c, hcomm.data(), N, G.C, directed, orig != nullptr, force_relabel, lay, packed_req);
    if (!lay.relabel) return;
    const DevBuf<i32> &d_order = c->sw_rl_order;
    std::vector<i32> &cm_mem = lay.cm_mem;
    c->sw_rl_emb.ensure((size_t)N * d);
    c->sw_rl_vec.ensure((size_t)4 * N);
    c->sw_rl_comm.ensure(N);
    k_permute_rows(c, G.emb, d_order.p, N, d, c->sw_rl_emb.p);
    G.emb = c->sw_rl_emb.p;
    double *v = c->sw_rl_vec.p;
    if (G.dist) { k_permute_rows(c, G.dist, d_order.p, N, 1, v); G.dist = v; }
    if (G.vw) { k_permute_rows(c, G.vw, d_order.p, N, 1, v + N); G.vw = v + N; }
    if (G.deg_in) { k_permute_rows(c, G.deg_in, d_order.p, N, 1, v + 2 * N); G.deg_in = v + 2 * N; }
    if (G.deg_out) { k_permute_rows(c, G.deg_out, d_order.p, N, 1, v + 3 * N); G.deg_out = v + 3 * N; }
    k_permute_i32(c, G.comm, d_order.p, N, c->sw_rl_comm.p);
    G.comm = c->sw_rl_comm.p;
    for (i64 q = 0; q < N; q++) cm_mem[q] = (i32)q; // the member lists in the new numbering (the old ones sit in the staging buffer)
}

// The community tables of a layout for the device (sw_cm_off, sw_cm_mem, sw_cm_pos), on the caller's packer; cm_pos is the
// caller's, since the packer reads it at its flush.  Shared by the sweep and the testing hook cge_vect_b_test.
void community_tables(cge_ctx *c, const SweepLayout &lay, i64 N, i64 C, WordPacker &pk, std::vector<i32> &cm_pos) {
    c->sw_cm_off.ensure(C + 1);
    c->sw_cm_mem.ensure(N);
    pk.add(c->sw_cm_off.p, lay.cm_off.data(), C + 1);
    pk.add(c->sw_cm_mem.p, lay.cm_mem.data(), N);
    cm_pos.resize(N); // position of every vertex in the community-sorted list
    for (i64 q = 0; q < N; q++) cm_pos[lay.cm_mem[q]] = (i32)q;
    c->sw_cm_pos.ensure(N);
    pk.add(c->sw_cm_pos.p, cm_pos.data(), N);
}

// D and its normalisation (:79-93 / :359-375), the community tables on the device, the starting T (:118) / Tin, Tout
// (:399-402), and TT, the three parts T rotates through in an undirected sweep.  Returns TT's leading dimension.
// packed: only lo, hi -- D is never stored; every alpha makes its GD from the embedding rows (k_packed_gd).
i64 prepare_distances(cge_ctx *c, const ScoreGraph &G, const SweepLayout &lay, int directed, bool packed) {
    const i64 N = G.N, C = G.C;
    hipStream_t st = c->stream;
    double *D = c->sw_D.p, *T1 = c->sw_T1.p, *T2 = c->sw_T2.p;
    if (packed)
        k_packed_extrema(c, G.emb, G.dist, N, G.d, c->sw_lohi.p);
    else {
        k_dist_matrix(c, G.emb, G.dist, N, G.d, D);
        k_minmax_upper(c, D, N, c->sw_lohi.p);
        k_normalise(c, D, N, c->sw_lohi.p);
    }
    WordPacker pk(c);
    std::vector<i32> cm_pos;
    community_tables(c, lay, N, C, pk, cm_pos);
    const std::vector<double> ones(N, 1.0); // T (:118)
    if (!directed) { // (the directed sweep reads the degrees back first, below)
        pk.add(T1, ones.data(), N);
        pk.add(T2, ones.data(), N);
    }
    pk.flush();
    if (c->bvec_blocks && !directed) k_bins_prepare(c, c->sw_cm_off.p, N, C, lay.bt_total); // where every bin's tile partials sit
    if (directed) { // Tin / Tout: zero where the in- / out-degree is
        std::vector<double> din(N), dout(N), hTin(N, 1.0), hTout(N, 1.0);
        HIP_CHECK(hipMemcpyAsync(din.data(), G.deg_in, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(dout.data(), G.deg_out, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (i64 i = 0; i < N; i++) {
            if (din[i] == 0) hTin[i] = 0.0;
            if (dout[i] == 0) hTout[i] = 0.0;
        }
        pk.add(T1, hTin.data(), N);
        pk.add(T2, hTout.data(), N);
        pk.flush();
    }
    // undirected: T rotates through the three parts of TT (Tld doubles each, zero beyond N).  Three, so that T_0 of an alpha
    // survives the fit of the next alpha, which may be enqueued before this one is checked.
    DevBuf<double> &TT = c->fp_T;
    const i64 Tld = (N + 63) / 64 * 64;
    TT.ensure((size_t)3 * Tld);
    c->fp_Tsave.ensure(N);
    HIP_CHECK(hipMemsetAsync(TT.p, 0, sizeof(double) * 3 * Tld, st));
    HIP_CHECK(hipMemcpyAsync(TT.p, T1, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    return Tld;
}

// full_graph_D of a set's sampled pairs, normalised by hi (lo == 0) :104-114
static void pair_distances(cge_ctx *c, const OrigView &orig, i64 d, i64 S, DevSamples &ds) {
    ds.dpos.ensure(S); ds.dneg.ensure(S);
    sampled_pair_dist(c, orig.Xr, d, ds.pi.p, ds.pj.p, S, orig.hi, ds.dpos.p);
    sampled_pair_dist(c, orig.Xr, d, ds.ni.p, ds.nj.p, S, orig.hi, ds.dneg.p);
}

// The samples to the device (c->dsets, one DevSamples per set): the sampled edges of the graph the local score samples from,
// their weights and, in landmark mode, full_graph_D of the sampled pairs.  `remap` (a relabelled exact-mode sweep): the pairs
// go into the sweep's numbering.
static void samples_to_device(cge_ctx *c, const SampleSet &smp, i64 N, i64 d, const OrigView *orig, const i32 *ex_src,
                              const i32 *ex_dst, const double *ex_hw, i64 ex_m, int directed, const i32 *remap) {
    hipStream_t st = c->stream;
    const bool landmarks = orig != nullptr;
    const i64 S = smp.S;
    const i32 *e_src = landmarks ? orig->src : ex_src, *e_dst = landmarks ? orig->dst : ex_dst;
    const double *e_hw = landmarks ? orig->h_w : ex_hw;
    const i64 e_m = landmarks ? orig->m : ex_m;
    std::vector<std::unique_ptr<DevSamples>> &dsets = c->dsets; // grow-only buffers kept by the context
    while ((i64)dsets.size() < smp.n_sets) dsets.emplace_back(new DevSamples());
    if (smp.on_device) { // library-drawn samples of the resident graph: everything stays on the device
        for (i64 t = 0; t < smp.n_sets; t++) {
            DevSamples &ds = *dsets[t];
            ds.pi.ensure(S); ds.pj.ensure(S); ds.ni.ensure(S); ds.nj.ensure(S); ds.wts.ensure(S);
            const i32 *pos = smp.d_pos.p + t * S;
            const i32 *pos_pairs = (directed && !landmarks && smp.d_pos2.p) ? smp.d_pos2.p + t * S : pos; // the overwriting draw (:510)
            k_prep_samples(c, pos, pos_pairs, smp.d_ni.p + t * S, smp.d_nj.p + t * S, e_src, e_dst, c->w.p, S, directed, ds.pi.p,
                           ds.pj.p, ds.ni.p, ds.nj.p, ds.wts.p);
            if (landmarks) pair_distances(c, *orig, d, S, ds);
        }
    } else {
        DevBuf<i32> d_idx, d_tmp;
        std::vector<i64> rows0(S);
        std::vector<i32> hs, hd;
        for (i64 t = 0; t < smp.n_sets; t++) {
            DevSamples &ds = *dsets[t];
            for (i64 k = 0; k < S; k++) {
                rows0[k] = smp.pos_idx[t * S + k] - 1;
                if (rows0[k] < 0 || rows0[k] >= e_m) CGE_THROW(CGE_E_ARG, "positive sample row out of range");
            }
            gather_rows(c, e_src, rows0, hs, d_idx, d_tmp);
            gather_rows(c, e_dst, rows0, hd, d_idx, d_tmp);
            std::vector<double> wts(S);
            for (i64 k = 0; k < S; k++) wts[k] = e_hw ? e_hw[rows0[k]] : 1.0;
            if (directed && !landmarks && !smp.pos_idx2.empty()) { // the overwriting second draw (:510)
                for (i64 k = 0; k < S; k++) rows0[k] = smp.pos_idx2[t * S + k] - 1;
                gather_rows(c, e_src, rows0, hs, d_idx, d_tmp);
                gather_rows(c, e_dst, rows0, hd, d_idx, d_tmp);
            }
            std::vector<i32> pi(S), pj(S), ni(S), nj(S);
            for (i64 k = 0; k < S; k++) {
                i32 a = hs[k], b = hd[k];
                if (!directed && a > b) std::swap(a, b); // E tuple (min,max) :133
                pi[k] = a; pj[k] = b;
                i64 u = smp.neg_i[t * S + k] - 1, v = smp.neg_j[t * S + k] - 1;
                if (!directed && u > v) std::swap(u, v);
                const i64 lim = landmarks ? orig->n : N;
                if (u < 0 || v < 0 || u >= lim || v >= lim) CGE_THROW(CGE_E_ARG, "negative sample out of range");
                ni[k] = (i32)u; nj[k] = (i32)v;
            }
            ds.pi.ensure(S); ds.pj.ensure(S); ds.ni.ensure(S); ds.nj.ensure(S); ds.wts.ensure(S);
            HIP_CHECK(hipMemcpyAsync(ds.pi.p, pi.data(), sizeof(i32) * S, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(ds.pj.p, pj.data(), sizeof(i32) * S, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(ds.ni.p, ni.data(), sizeof(i32) * S, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(ds.nj.p, nj.data(), sizeof(i32) * S, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(ds.wts.p, wts.data(), sizeof(double) * S, hipMemcpyHostToDevice, st));
            if (landmarks) pair_distances(c, *orig, d, S, ds);
            HIP_CHECK(hipStreamSynchronize(st)); // host vectors go out of scope
        }
    }
    if (remap) // the sampled pairs index the score graph: into the new numbering (GD is a full symmetric matrix here)
        for (i64 t = 0; t < smp.n_sets; t++) {
            DevSamples &ds = *dsets[t];
            k_remap_i32(c, ds.pi.p, remap, S);
            k_remap_i32(c, ds.pj.p, remap, S);
            k_remap_i32(c, ds.ni.p, remap, S);
            k_remap_i32(c, ds.nj.p, remap, S);
        }
}

// The fused chain's tables, one per sample set (host copies in h_epi; the device copies, which the fit's epilogue loads after
// its loop, in c->sw_fused_epi).  The local score tallies the samples [s0, s1) of every set; fuse_auc: on the fit's launch.
// One table without the prepared tally operands: vect_B's half from the context's tile tables (comm: the communities in the
// sweep's numbering) and the S samples' distances and weights.  Shared by fused_tables and the testing hook cge_fused_chain_test,
// whose caller supplies the prepared operands.
cge_fit_fused fused_entry(cge_ctx *c, const i32 *comm, i64 S, const double *dpos, const double *dneg, const double *wts) {
    cge_fit_fused e{};
    e.comm = comm; e.fc = c->sw_bt_fc.p; e.ns = c->sw_bt_ns.p; e.base = c->sw_bt_base.p; e.partial = c->sw_bt_part.p;
    e.S = S;
    e.dpos = dpos; e.dneg = dneg; e.wts = wts;
    e.auc_part = c->sw_scal.p + RES_AUC;
    return e;
}
// the tables' device copies (c->sw_fused_epi), which the fit's epilogue loads after its loop
void fused_upload(cge_ctx *c, const std::vector<cge_fit_fused> &h_epi) {
    c->sw_fused_epi.ensure(h_epi.size() * sizeof(cge_fit_fused));
    static_assert(sizeof(cge_fit_fused) % 8 == 0, "packed as 4-byte words");
    WordPacker pk(c);
    pk.add(reinterpret_cast<i32 *>(c->sw_fused_epi.p), reinterpret_cast<const i32 *>(h_epi.data()),
           (i64)(h_epi.size() * sizeof(cge_fit_fused) / 4));
    pk.flush();
}
void fused_tables(cge_ctx *c, const ScoreGraph &G, const OrigView *orig, const i32 *old2new, i64 n_sets, i64 s0, i64 s1,
                  bool fuse_auc, std::vector<cge_fit_fused> &h_epi) {
    h_epi.resize(n_sets);
    for (i64 t = 0; t < n_sets; t++) {
        DevSamples &ds = *c->dsets[t];
        cge_fit_fused &e = h_epi[t];
        e = fused_entry(c, G.comm, s1 - s0, ds.dpos.p + s0, ds.dneg.p + s0, ds.wts.p + s0);
        if (fuse_auc && e.S > 0) { // everything of the tally that depends neither on alpha nor on T, once
            ds.aidx.ensure((size_t)4 * e.S); ds.afac.ensure((size_t)8 * e.S + CGE_PARTIAL_BLOCKS);
            c->sw_fused_pw.ensure((size_t)2 * e.S);
            k_auc_prepare(c, orig->v2l, old2new, orig->vw, orig->lweight, ds.pi.p + s0, ds.pj.p + s0, ds.ni.p + s0,
                          ds.nj.p + s0, e.wts, e.S, ds.aidx.p, ds.afac.p, ds.afac.p + 8 * e.S);
            e.aidx = ds.aidx.p; e.afac = ds.afac.p; e.aden = ds.afac.p + 8 * e.S; e.apw = c->sw_fused_pw.p;
        }
    }
    fused_upload(c, h_epi);
}

// cge_score_batch: a sweep on the fused path is prepared here and run by the batch, beside other members' sweeps
// (batch_host.cpp); what its alphas read moves out of the context into the hand-off, everything else stays scratch.
// False: its fit does not share a launch (the sweep runs here).
static bool hand_off(cge_ctx *c, SweepHandoff &h, const ScoreGraph &G, const SampleSet &smp, int split, i64 Tld,
                     std::vector<cge_fit_fused> &h_epi) {
    const i64 N = G.N, vlen = packed_len(G.C);
    FlowGeometry geo;
    if (!flow_batch_member(N, device_cus(c), false, &geo) || geo.G > h.max_G || !k_fit_flow_multi_fits(geo.NW, false)) return false;
    hipStream_t st = c->stream;
    k_pow_prepare(c, c->sw_D.p, N, true, true);
    h.Lh.swap(c->sw_Lh); h.Ll.swap(c->sw_Ll);
    c->pow_logs_N = c->pow_logs_blocked_N = 0; // (the context's logarithm left with the hand-off)
    h.comm.swap(c->sw_rl_comm); h.vw.swap(c->sw_rl_vec);
    h.bt_fc.swap(c->sw_bt_fc); h.bt_ns.swap(c->sw_bt_ns); h.bt_base.swap(c->sw_bt_base); h.bt_part.swap(c->sw_bt_part);
    h.cm_off.swap(c->sw_cm_off); h.fused_pw.swap(c->sw_fused_pw);
    h.dsets.clear();
    for (i64 t = 0; t < smp.n_sets; t++) {
        h.dsets.emplace_back(std::move(c->dsets[t]));
        c->dsets[t].reset(new DevSamples());
    }
    h.vectC.ensure(vlen); // (the context's vect_C is landmark state of the member: copied)
    HIP_CHECK(hipMemcpyAsync(h.vectC.p, G.vectC, sizeof(double) * vlen, hipMemcpyDeviceToDevice, st));
    h.T.ensure((size_t)3 * Tld); // T rotates through three parts (as TT); T_0 = ones
    HIP_CHECK(hipMemcpyAsync(h.T.p, c->fp_T.p, sizeof(double) * 3 * Tld, hipMemcpyDeviceToDevice, st));
    h.N = N; h.C = G.C; h.S = smp.S; h.n_sets = smp.n_sets; h.Tld = Tld; h.split = split;
    h.geo = geo;
    h.h_epi = std::move(h_epi);
    h.w = G.vw;
    h.deferred = true;
    HIP_CHECK(hipStreamSynchronize(st)); // (the staging packer's host memory)
    return true;
}

// The directed sibling of hand_off: the sweep is prepared (prepare_distances, samples_to_device) and its alphas are run by the
// batch (batch_host.cpp: host_batch_sweep).  What they read moves out of the context -- D, the logarithm, the community tables,
// the prepared sample sets -- or, where it is landmark state that the next member's landmark phase overwrites, is copied:
// Tin / Tout, the degrees, vect_C, v2l and the landmarks' weights.  False: the fit shares no launch (the sweep runs here).
static bool hand_off_directed(cge_ctx *c, SweepHandoff &h, const ScoreGraph &G, const OrigView &orig, const SampleSet &smp, int split) {
    const i64 N = G.N, C = G.C, vlen = C * C;
    // (a directed member shares the launch on the geometry of its own k_fit_persistent_dir launch: one quarter block per
    // workgroup, which the multi kernel exists for, and no more than half the chip, so that a launch holds two members at least)
    FlowGeometry geo;
    if (!flow_batch_member(N, device_cus(c), true, &geo) || geo.G > h.max_G || !k_fit_flow_multi_fits(geo.NW, true)) return false;
    hipStream_t st = c->stream;
    k_pow_prepare(c, c->sw_D.p, N, false); // what the sweep does once before its first alpha
    h.logs = c->pow_logs_N == N && !c->pow_logs_upper; // (k_pow_matrix's own rule for whole rows)
    if (h.logs) { h.Lh.swap(c->sw_Lh); h.Ll.swap(c->sw_Ll); }
    c->pow_logs_N = c->pow_logs_blocked_N = 0; // (the context's logarithm left with the hand-off)
    h.D.swap(c->sw_D);
    h.GD.ensure((size_t)N * N);
    h.cm_off.swap(c->sw_cm_off); h.cm_mem.swap(c->sw_cm_mem); h.cm_pos.swap(c->sw_cm_pos);
    h.bvec_form = k_bvec_form(c, N);
    h.dsets.clear();
    for (i64 t = 0; t < smp.n_sets; t++) {
        h.dsets.emplace_back(std::move(c->dsets[t]));
        c->dsets[t].reset(new DevSamples());
    }
    h.vectC.ensure(vlen);
    h.Tio.ensure((size_t)2 * N); h.deg.ensure((size_t)2 * N); h.lweight.ensure(N); h.v2l.ensure(orig.n);
    HIP_CHECK(hipMemcpyAsync(h.vectC.p, G.vectC, sizeof(double) * vlen, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h.Tio.p, c->sw_T1.p, sizeof(double) * N, hipMemcpyDeviceToDevice, st)); // Tin, Tout (zero where the degree is)
    HIP_CHECK(hipMemcpyAsync(h.Tio.p + N, c->sw_T2.p, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h.deg.p, G.deg_in, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h.deg.p + N, G.deg_out, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h.lweight.p, orig.lweight, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h.v2l.p, orig.v2l, sizeof(i32) * orig.n, hipMemcpyDeviceToDevice, st));
    h.N = N; h.C = C; h.S = smp.S; h.n_sets = smp.n_sets; h.Tld = (i64)geo.Nt * 64; h.split = split;
    h.geo = geo;
    h.directed = true;
    h.deferred = true;
    HIP_CHECK(hipStreamSynchronize(st)); // (the staging packer's host memory)
    return true;
}

// ---- one alpha -------------------------------------------------------------------------------------

// Whether a sweep starts on the persistent form of its fit (the geometry is asked at the first launch)
bool persistent_wanted(const cge_ctx *c, i64 N) {
    return !c->fit_persistent_broken && c->opt_fit_persistent != 1 && (c->opt_fit_persistent >= 2 || N >= 128);
}

// One launch (pair) per iteration: `launch(k)` enqueues iteration k, in batches -- the first as long as the previous fit, at
// most 32 from then on.  After each batch the host reads the fit's flags ([0] done, [1] iterations) and, when `ring` is given,
// the changes of the fit's last iterations (ring_len of them: 3 undirected, 4 by the directed tile pair).  Returns the iterations.
template <class Launch>
static i64 fit_by_launches(cge_ctx *c, i64 prev_iters, double alpha, double delta, const int *flags,
                           const unsigned long long *ring, Launch launch, int ring_len = 3) {
    hipStream_t st = c->stream;
    i64 batch = std::max<i64>(4, std::min<i64>(prev_iters, 128));
    for (i64 k = 0;;) {
        for (i64 b = 0; b < batch; b++, k++) launch(k);
        int hf[2];
        unsigned long long hr[4];
        HIP_CHECK(hipMemcpyAsync(hf, flags, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
        if (ring) HIP_CHECK(hipMemcpyAsync(hr, ring, sizeof(unsigned long long) * ring_len, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const i64 iters = hf[1];
        if (hf[0]) return iters;
        if (ring) {
            double flast;
            std::memcpy(&flast, &hr[(k - 1) % ring_len], sizeof(double));
            if (!(flast > delta)) return iters; // the last launch of the batch was the converging iteration (iters == k)
        }
        if (iters > c->opt_fit_max_iters) CGE_THROW(CGE_E_ASSERT, "Chung-Lu fit did not converge at alpha=%g (%lld iterations; the reference's `while diff > delta` would not return)", alpha, (long long)iters);
        batch = std::max<i64>(4, std::min<i64>(batch, 32));
    }
}

// The undirected fit of one alpha from T_0 = part fit.tpar of TT.  The persistent form (GD's upper triangle in registers,
// kernels_fitp.hip) is only enqueued -- with the rest of the alpha's chain riding on it when `ff` is given (ff_dev: its
// device copy) -- and its verdict is looked at when the alpha is collected; else one launch per iteration (k_fit_sym_step,
// over the upper tiles only).  `upper`: GD's upper triangle suffices (the power matrix made here when the fused launch does not
// apply after all).  `packed`: the matrix is the upper tiles in sw_PK (never persistent).
void fit_undirected(cge_ctx *c, i64 N, const double *w, i64 Tld, double alpha, bool upper, bool packed,
                    const cge_fit_fused *ff, const cge_fit_fused *ff_dev, FitForm &fit, AlphaSlot &sl) {
    hipStream_t st = c->stream;
    double *const GD = packed ? c->sw_PK.p : c->sw_GD.p, *const TT = c->fp_T.p;
    int *flags = c->sw_flags.p;
    if (!fit.persistent) HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int) * 4, st));
    sl.t0_par = fit.tpar;
    if (fit.persistent) {
        const int tnext = (fit.tpar + 1) % 3;
        if (k_fit_flow_enqueue(c, ff ? nullptr : GD, N, TT + (i64)fit.tpar * Tld, TT + (i64)tnext * Tld, Tld, w, fit.eps,
                               fit.delta, (int *)(c->sw_scal.p + RES_FIT), ff, ff_dev)) {
            sl.fused = ff != nullptr;
            sl.fit_async = true;
            fit.tpar = tnext;
            return;
        }
        fit.persistent = false; // the register-resident form does not apply to this size: one launch per iteration from here on
        if (ff) { // (the fused launch was to supply the matrix)
            k_pow_prepare(c, c->sw_D.p, N, upper);
            k_pow_matrix(c, c->sw_D.p, N, alpha, GD, upper);
        }
        HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int) * 4, st));
    }
    // T alternates between two parts of TT
    HIP_CHECK(hipMemsetAsync(c->sw_fring.p, 0, sizeof(unsigned long long) * 4, st));
    double *Tb2[2] = {TT + (i64)fit.tpar * Tld, TT + (i64)((fit.tpar + 1) % 3) * Tld};
    c->sweep_used_fp_P = true;
    sl.iters = fit_by_launches(c, fit.prev_iters, alpha, fit.delta, flags, c->sw_fring.p, [&](i64 k) {
        k_fit_sym_step(c, GD, Tb2[k & 1], Tb2[(k + 1) & 1], w, N, fit.eps, fit.delta, (int)k, c->sw_fring.p, flags, flags + 1,
                       packed);
    });
    if (sl.iters & 1) fit.tpar = (fit.tpar + 1) % 3;
}

// The directed fit of one alpha, Tin / Tout (sw_T1 / sw_T2) updated in place: the whole fit in one launch (kernels_fitp.hip) or
// one launch pair per iteration.  The default persistent form is only enqueued: the rest of the alpha's chain is queued behind
// it and its verdict arrives with the alpha's scalars (Tin / Tout are written on success only, so a failed launch is redone
// from the same iterates with one launch pair per iteration).
void fit_directed(cge_ctx *c, const ScoreGraph &G, double alpha, FitForm &fit, AlphaSlot &sl) {
    hipStream_t st = c->stream;
    const i64 N = G.N;
    const double *GD = fit.dir_tiles == 2 ? c->sw_PK.p : c->sw_GD.p;
    double *Tin = c->sw_T1.p, *Tout = c->sw_T2.p;
    int *flags = c->sw_flags.p;
    HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int) * 4, st));
    const double init[2] = {fit.eps, 1.0}; // epsilon, diff (:434-435)
    HIP_CHECK(hipMemcpyAsync(c->sw_fitstate.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    bool enqueued_only = false;
    if (fit.persistent_dir && k_fit_persistent_dir(c, GD, N, Tin, Tout, G.deg_in, G.deg_out, fit.eps, 1.0, fit.delta,
                                                   &sl.iters, (int *)(c->sw_scal.p + RES_FIT), &enqueued_only)) {
        if (enqueued_only) sl.fit_async = true;
        else c->stat_fit_persistent++;
        return;
    }
    if (fit.persistent_dir) { // abandoned: Tin / Tout are untouched; one launch pair per iteration from here on
        fit.persistent_dir = false;
        HIP_CHECK(hipMemsetAsync(flags, 0, sizeof(int) * 4, st));
    }
    if (fit.dir_tiles) {
        // by the tile pair (kernels_fitp.hip): every upper tile read once per iteration.  The iterates alternate between
        // (sw_T1, sw_T2) and the two halves of fp_Td; an odd count leaves the result in the latter, which is copied home.
        // f travels in a ring of four, epsilon in the first two doubles of sw_fitstate.
        c->fp_Td.ensure((size_t)2 * N);
        c->sweep_used_fp_P = true;
        HIP_CHECK(hipMemsetAsync(c->sw_fring.p, 0, sizeof(unsigned long long) * 4, st));
        double *Ti[2] = {Tin, c->fp_Td.p}, *To[2] = {Tout, c->fp_Td.p + N};
        sl.iters = fit_by_launches(c, fit.prev_iters, alpha, fit.delta, flags, c->sw_fring.p, [&](i64 k) {
            k_fit_sym_dir_step(c, GD, Ti[k & 1], To[k & 1], Ti[(k + 1) & 1], To[(k + 1) & 1], G.deg_in, G.deg_out, N, fit.eps, 1.0,
                               fit.delta, (int)k, c->sw_fring.p, c->sw_fitstate.p, flags, flags + 1, fit.dir_tiles == 2);
        }, 4);
        if (sl.iters & 1) {
            HIP_CHECK(hipMemcpyAsync(Tin, Ti[1], sizeof(double) * N, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(Tout, To[1], sizeof(double) * N, hipMemcpyDeviceToDevice, st));
        }
        return;
    }
    sl.iters = fit_by_launches(c, fit.prev_iters, alpha, fit.delta, flags, nullptr, [&](i64) {
        k_fit_symv_dir(c, GD, Tin, Tout, N, c->sw_S1.p, c->sw_S2.p, flags);
        k_fit_update_dir(c, Tin, Tout, c->sw_S1.p, c->sw_S2.p, G.deg_in, G.deg_out, N, fit.delta, flags, flags + 1,
                         c->sw_fitstate.p);
    });
}

// An enqueued persistent fit was abandoned: what was enqueued behind it is drained, and this fit and every later one of the
// sweep go by one launch per iteration -- this one again from its T_0, which is still in place.
void leave_persistent(cge_ctx *c, int directed, FitForm &fit, const AlphaSlot &sl) {
    HIP_CHECK(hipStreamSynchronize(c->stream));
    note_fit_fallback(c);
    if (directed) fit.persistent_dir = false;
    else {
        fit.persistent = false;
        fit.tpar = sl.t0_par;
    }
}

// The local score's tallies of one alpha (samples [s0, s1) of `ds`: this rank's share) into the block partials of the scalars.
// Landmark mode reads T through the landmark ids of the original numbering: a relabelled sweep (old2new) un-permutes it first.
static void local_score_tallies(cge_ctx *c, const double *Ta, const double *Tb, i64 N, int directed, const OrigView *orig,
                                const i32 *old2new, const DevSamples &ds, i64 s0, i64 s1, double alpha, bool packed) {
    double *part = c->sw_scal.p + RES_AUC;
    if (!orig) {
        k_auc_exact(c, packed ? c->sw_PK.p : c->sw_GD.p, Ta, Tb, N, ds.pi.p + s0, ds.pj.p + s0, ds.ni.p + s0, ds.nj.p + s0,
                    ds.wts.p + s0, s1 - s0, nullptr, part, packed);
        return;
    }
    if (old2new) {
        c->sw_rl_T.ensure((size_t)2 * N);
        k_permute_rows(c, Ta, old2new, N, 1, c->sw_rl_T.p);
        Ta = c->sw_rl_T.p;
        if (directed) {
            k_permute_rows(c, Tb, old2new, N, 1, c->sw_rl_T.p + N);
            Tb = c->sw_rl_T.p + N;
        } else
            Tb = Ta;
    }
    k_auc_landmark(c, Ta, Tb, orig->v2l, orig->vw, orig->lweight, ds.pi.p + s0, ds.pj.p + s0, ds.ni.p + s0, ds.nj.p + s0,
                   ds.dpos.p + s0, ds.dneg.p + s0, ds.wts.p + s0, s1 - s0, alpha, nullptr, part);
}

// vect_B and its divergence(s) of one alpha (want_div), then the alpha's scalars to pinned slot `slot` and an event.
// bvec_partials: vect_B's tile partials came with the fit.  arm: the next alpha's persistent fit may take its hand-off slots
// armed by this alpha's last launch.  packed: GD is the upper tiles in sw_PK (vect_B goes by tiles then).
static void divergence_and_copy_out(cge_ctx *c, const ScoreGraph &G, int directed, int split, const double *Ta,
                                    const double *Tb, bool want_div, bool bvec_partials, bool arm, i64 Tld, int slot, bool packed) {
    hipStream_t st = c->stream;
    const i64 N = G.N, C = G.C, vlen = directed ? C * C : packed_len(C);
    const double *GD = packed ? c->sw_PK.p : c->sw_GD.p;
    if (packed && want_div && !(c->bvec_blocks && !c->opt_test_bvec_plain))
        CGE_THROW(CGE_E_ASSERT, "packed exact sweep without the tile form of vect_B");
    const i32 *cm_off = c->sw_cm_off.p;
    double *scal = c->sw_scal.p, *vectB = c->sw_vectB.p, *host_out = c->pin_scal.p + RES_STRIDE * slot;
    if (want_div && (bvec_partials || c->bvec_blocks) && !directed && !c->opt_test_bvec_plain) {
        // tile partials (from the fit's epilogue, or one pass over GD) -> vect_B and its divergence(s) in one launch
        if (!bvec_partials) k_bvec_tiles(c, GD, Ta, Tb, cm_off, N, directed, packed);
        // the last launch of the alpha: it also hands the alpha's scalars to the host's pinned slot and arms the hand-off
        // slots of the next alpha's persistent fit (instead of a copy and a fill of their own)
        cge_chain_tail tail{};
        tail.host_out = host_out;
        tail.scal = scal;
        tail.res_js = (int)RES_JS;
        tail.res_len = (int)RES_LEN;
        const bool arms = arm && k_fit_flow_arm_region(c, N, Tld, &tail.arm, &tail.arm_n16, &tail.arm_word);
        if (!arms) { tail.arm = nullptr; tail.arm_n16 = 0; }
        k_bins_js(c, cm_off, N, C, G.vectC, vectB, split ? 2 : 1, scal + RES_JS, &tail);
        if (arms) c->flow_armed_words = 4 * tail.arm_n16;
    } else {
        if (want_div) {
            if (bvec_partials) k_bvec_bins(c, cm_off, N, C, directed, vectB); // the tile partials came with the fit
            else if (packed) { // (directed) the stored tiles and their mirrors, then the C^2 bins
                k_bvec_tiles(c, GD, Ta, Tb, cm_off, N, directed, true);
                k_bvec_bins(c, cm_off, N, C, directed, vectB);
            } else k_bvec(c, GD, Ta, Tb, c->sw_cm_pos.p, cm_off, c->sw_cm_mem.p, N, C, directed, c->sw_rowbins.p, vectB);
            if (!split)
                k_js(c, G.vectC, vectB, vlen, C, directed, 0, nullptr, scal + RES_JS);
            else {
                k_js(c, G.vectC, vectB, vlen, C, directed, 1, nullptr, scal + RES_JS);
                k_js(c, G.vectC, vectB, vlen, C, directed, 2, nullptr, scal + RES_JS + CGE_PARTIAL_BLOCKS);
            }
        }
        // the block partials of the alpha's reductions and (behind them) the verdict of an enqueued fit, one copy; the host
        // adds the partials in block order -- what the one-thread "final" kernels did, without their launches
        HIP_CHECK(hipMemcpyAsync(host_out, scal, sizeof(double) * RES_LEN, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipEventRecord(c->sweep_ev[slot], st));
}

// What the alphas of one sweep read: the score graph in the sweep's numbering and what its set-up decided
struct SweepView {
    const ScoreGraph &G;
    const OrigView *orig; // landmark mode
    int directed, split;
    i64 Tld;
    const i32 *old2new;   // a relabelled sweep: a vertex's number in the sweep
    bool fuse, fuse_auc;  // the rest of the chain rides on the fit's launch; the local score's tallies too
    const std::vector<cge_fit_fused> &h_epi;
    i64 n_sets, s0, s1;   // sample sets; this rank's samples of each
    bool shard;           // the tallies are split over the ranks
    bool packed;          // an exact sweep on the upper tiles of the current alpha's GD alone (sw_PK)
};

// One alpha's chain on the stream: pow, the fit, the local score's tallies, vect_B, JS, the scalars -> pinned slot (ia mod 2), an
// event.  With the enqueue-only persistent fit nothing in the chain needs the host, so the sweep enqueues alpha i + 1 before it
// waits for alpha i.
static void enqueue_alpha(cge_ctx *c, const SweepView &sw, i64 ia, bool want_auc, bool want_div, FitForm &fit, AlphaSlot &sl) {
    const ScoreGraph &G = sw.G;
    const i64 N = G.N, set = sw.n_sets == 1 ? 0 : ia - 1;
    const double alpha = AlphaBook::AlphaStep * (double)ia;
    // the undirected persistent fit and vect_B read the upper triangle only; the exact-mode AUC, the directed vect_B
    // and the launch-per-iteration fits read whole rows
    const bool upper = sw.orig && !sw.directed;
    sl = AlphaSlot();
    const bool fused_now = sw.fuse && fit.persistent && c->pow_logs_blocked_N == N; // (a fallback in mid-sweep ends it: the matrix is needed then)
    if (sw.fuse && !fused_now && c->pow_logs_N != N) k_pow_prepare(c, c->sw_D.p, N, upper); // (left the fused path: the row-major logarithm)
    if (sw.packed) k_packed_gd(c, G.emb, G.dist, N, G.d, c->sw_lohi.p, alpha, c->opt_pow_exp2, c->sw_PK.p);
    else if (!fused_now) k_pow_matrix(c, c->sw_D.p, N, alpha, c->sw_GD.p, upper);
    cge_fit_fused ff{};
    if (fused_now) { // this alpha's copy of the epilogue table: what is not wanted is left out
        ff = sw.h_epi[set];
        ff.Lh = c->sw_Lh.p; ff.Ll = c->sw_Ll.p; ff.alpha = alpha;
        if (!want_div) ff.partial = nullptr;
        if (!(want_auc && sw.fuse_auc)) ff.auc_part = nullptr;
    }
    if (!sw.directed)
        fit_undirected(c, N, G.vw, sw.Tld, alpha, upper, sw.packed, fused_now ? &ff : nullptr,
                       fused_now ? reinterpret_cast<const cge_fit_fused *>(c->sw_fused_epi.p) + set : nullptr, fit, sl);
    else
        fit_directed(c, G, alpha, fit, sl);
    if (!sl.fit_async) fit.prev_iters = sl.iters;
    const double *Tcur = c->fp_T.p + (i64)fit.tpar * sw.Tld;
    const double *Ta = sw.directed ? c->sw_T2.p : Tcur, *Tb = sw.directed ? c->sw_T1.p : Tcur; // (Tout, Tin)
    sl.Ta = Ta; sl.Tb = Tb;
    if (want_auc && !(sl.fused && ff.auc_part))
        local_score_tallies(c, Ta, Tb, N, sw.directed, sw.orig, sw.old2new, *c->dsets[set], sw.s0, sw.s1, alpha, sw.packed);
    if (sw.shard) {
        // The verdict of an enqueued fit is rank-local (a hand-off may time out on one rank only), but a redo re-issues
        // this exchange and changes what the rank enqueues from then on: the ranks must take it together.  So the verdict
        // rides along as one more summand -- at EVERY alpha of a sweep with split tallies, with or without a local score --
        // and every rank redoes the alpha when any rank's fit was abandoned: the ranks never leave lock-step.
        double *scal = c->sw_scal.p;
        k_fit_verdict(c, (const int *)(scal + RES_FIT), sl.fit_async ? 1 : 0, scal + RES_VERD);
        sl.shared_verdict = true;
        if (want_auc) cge_allreduce_dev(c, scal + RES_AUC, 2 * CGE_PARTIAL_BLOCKS + 1, 0);
        else cge_allreduce_dev(c, scal + RES_VERD, 1, 0);
    }
    divergence_and_copy_out(c, G, sw.directed, sw.split, Ta, Tb, want_div, sl.fused && ff.partial,
                            fit.persistent && ia < AlphaBook::n_alpha, sw.Tld, (int)(ia & 1), sw.packed);
}

// ---- the sweep -------------------------------------------------------------------------------------

// The packed form's two O(N^2) buffers: the upper tiles of GD (sw_PK) and the fit's partial vectors (fp_P).  What the context still
// holds of the resident form from earlier sweeps -- D, GD, the logarithm -- is released first, so that a context that scored a
// smaller graph can score a large one; then whatever has to grow must fit the free memory.
// (directed: two sets of partial vectors, toward Sin and toward Sout)
static void packed_buffers(cge_ctx *c, i64 N, int directed) {
    const i64 Nt = (N + 63) / 64, NT = Nt * (Nt + 1) / 2;
    const size_t pk_words = (size_t)NT * CGE_TILE_DOUBLES, fp_words = (size_t)Nt * Nt * 64 * (directed ? 2 : 1);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->sw_D.release(); c->sw_GD.release(); c->sw_Lh.release(); c->sw_Ll.release();
    c->pow_logs_N = c->pow_logs_blocked_N = 0;
    size_t need = 0;
    if (c->sw_PK.n < pk_words) { c->sw_PK.release(); need += pk_words * sizeof(double); }
    if (c->fp_P.n < fp_words) { c->fp_P.release(); need += fp_words * sizeof(double); }
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        CGE_THROW(CGE_E_OOM, "exact sweep of %lld vertices: the packed matrix and the fit's partial vectors need %llu bytes, %llu are free",
                  (long long)N, (unsigned long long)need, (unsigned long long)free_b);
    c->sw_PK.ensure(pk_words);
    c->fp_P.ensure(fp_words);
}

void host_wgcl_sweep(cge_ctx *c, const ScoreGraph &G_in, const OrigView *orig, const i32 *ex_src, const i32 *ex_dst,
                     const double *ex_hw, i64 ex_m, int directed, int split, const SampleSet &smp, double out[7],
                     int *out_len, cge_trace *trace, SweepHandoff *defer) {
    ScoreGraph G = G_in; // the per-vertex arrays may be replaced by community-sorted copies (plan_layout)
    const i64 N = G.N, C = G.C, S = smp.S;
    const i64 vlen = directed ? C * C : packed_len(C);
    // The resident form keeps D, GD and (when they fit) the logarithm on the device; beyond its limit an undirected exact sweep
    // runs PACKED where that form applies (the tile form of vect_B: N >= 256, C >= 2, exact_relabel, the tile tables accept the
    // layout), option "exact_packed" = 1 wherever it applies.  A directed sweep stays resident, with the limit, unless option
    // "exact_packed_directed" allows the packed form: 1 beyond the limit, 2 wherever the form applies (the same conditions).
    const double resident_limit = c->opt_test_resident_limit > 0 ? c->opt_test_resident_limit : 200e9;
    const bool beyond = (double)N * (double)N * 8.0 * 2.2 > resident_limit;
    const bool packed_req = !orig && (directed ? c->opt_exact_packed_directed == 2 || (beyond && c->opt_exact_packed_directed == 1)
                                               : beyond || c->opt_exact_packed == 1);
    c->stat_exact_packed = 0;
    if (beyond && !packed_req) {
        if (directed && !orig)
            CGE_THROW(CGE_E_OOM, "score graph with %lld vertices does not fit (a directed exact sweep runs on the packed tiles only "
                      "under option exact_packed_directed)", (long long)N);
        CGE_THROW(CGE_E_OOM, "score graph with %lld vertices does not fit", (long long)N);
    }
    c->sw_T1.ensure(N); c->sw_T2.ensure(N); c->sw_S1.ensure(N); c->sw_S2.ensure(N);
    c->sw_rowbins.ensure((size_t)N * C);
    c->sw_vectB.ensure(vlen);
    c->sw_scal.ensure(RES_STRIDE); // an alpha's scalars (RES_*)
    c->sw_lohi.ensure(2);
    c->sw_fitstate.ensure(4);
    c->sw_flags.ensure(4); // [0]=done, [1]=iters
    c->sw_fring.ensure(4);

    SweepLayout lay;
    plan_layout(c, G, orig, directed, lay, packed_req);
    const bool packed = packed_req && c->bvec_blocks && !c->opt_test_bvec_plain;
    if (beyond && !packed)
        CGE_THROW(CGE_E_OOM, "score graph with %lld vertices does not fit (the packed form of an exact sweep does not apply to it)",
                  (long long)N);
    const i64 Nt64 = (N + 63) / 64;
    if (packed) packed_buffers(c, N, directed);
    else {
        c->sw_PK.release(); // (held only while packed sweeps run)
        c->sw_D.ensure((size_t)N * N);
        c->sw_GD.ensure((size_t)N * N);
    }
    c->sweep_used_fp_P = false;
    const i64 Tld = prepare_distances(c, G, lay, directed, packed);
    // sample tallies split over the ranks: with the in-library communicator (stream-ordered, no host synchronisation in the
    // enqueued chain) from 10^5 samples on; option "shard_samples" = 2 forces it (tests, also through the hook), 0 disables
    const bool shard = c->has_coll && S >= c->coll.world &&
                       (c->opt_shard_samples == 2 || (c->opt_shard_samples == 1 && c->rccl_comm && S >= 100000));
    fit_sweep_begin(c);
    FitForm fit;
    fit.persistent = !directed && !packed && persistent_wanted(c, N);
    fit.persistent_dir = directed && !packed && persistent_wanted(c, N);
    fit.dir_tiles = !directed ? 0 : packed ? 2 : c->opt_test_fit_dir_tiles ? 1 : 0;
    fit.eps = directed ? 0.9 : 0.25;
    c->stat_fit_persistent = 0;
    c->stat_fit_iters = 0;
    samples_to_device(c, smp, N, G.d, orig, ex_src, ex_dst, ex_hw, ex_m, directed,
                      lay.relabel && !orig ? lay.old2new.p : nullptr);
    // N > 1 with many samples: rank r tallies the samples [S r / W, S (r + 1) / W) and the block tallies are summed
    // over the ranks -- the same array on every rank afterwards, so all ranks take the same early stops
    const i64 s0 = shard ? S * c->coll.rank / c->coll.world : 0, s1 = shard ? S * (c->coll.rank + 1) / c->coll.world : S;
    const bool fuse_auc = orig && s1 - s0 < 65536 && s1 > s0; // (beyond: auc_landmark_kernel's wide form, as its own launch)
    std::vector<cge_fit_fused> h_epi;
    if (lay.fuse) fused_tables(c, G, orig, lay.old2new.p, smp.n_sets, s0, s1, fuse_auc, h_epi);
    c->stat_fit_fused = 0;
    if (defer) defer->deferred = false;
    if (defer && lay.fuse && fuse_auc && fit.persistent && !shard && !c->has_coll && hand_off(c, *defer, G, smp, split, Tld, h_epi))
        return;
    // a directed landmark-mode member: its fits share fit_flow_dir_multi_kernel's launch (no fused chain, so neither option
    // fit_fused nor the fused tallies' sample limit applies; a sweep relabelled for the tile form of vect_B runs here)
    if (defer && directed && orig && fit.persistent_dir && !shard && !c->has_coll && !lay.relabel && !c->bvec_blocks &&
        hand_off_directed(c, *defer, G, *orig, smp, split))
        return;

    // ---- alpha sweep: alpha i + 1 is enqueued before the host waits for alpha i, unless the sweep may end at alpha i (so
    // nothing is ever computed in vain) or the fit of alpha i needs the host
    // (Round 4 tried the next alpha's power matrix on a side stream beside this alpha's vect_B / JS / AUC: +0.65 ms, the two
    // cross-queue dependencies per alpha cost more than they hid -- profiles/r04_pow_overlap_ab.txt; removed in round 5, when
    // the power matrix moved into the fit's prologue anyway.)
    const SweepView sw{G, orig, directed, split, Tld, lay.old2new.p, lay.fuse, fuse_auc, h_epi, smp.n_sets, s0, s1, shard, packed};
    AlphaBook book(S, split, trace);
    AlphaSlot slots[2];
    c->pin_scal.ensure(2 * RES_STRIDE);
    // log2(1 - D) once for the whole sweep (the upper tiles only when every alpha reads only those); a fallback of the
    // persistent fit in mid-sweep makes k_pow_matrix use the library pow for the whole rows it then needs
    if (!packed) k_pow_prepare(c, c->sw_D.p, N, orig && !directed, lay.fuse);
    i64 next_enqueue = 1;
    for (i64 ia = 1; ia <= AlphaBook::n_alpha; ia++) {
        AlphaSlot &sl = slots[ia & 1];
        if (next_enqueue == ia) {
            enqueue_alpha(c, sw, ia, !book.skip_auc, !book.skip_div, fit, sl);
            next_enqueue = ia + 1;
        }
        // (directed: Tin / Tout are updated in place, so the next alpha is not queued before this one's verdict is known)
        if (sl.fit_async && !directed && !book.may_end_here() && ia < AlphaBook::n_alpha) { // keep the device busy meanwhile
            enqueue_alpha(c, sw, ia + 1, !book.skip_auc, !book.skip_div, fit, slots[(ia + 1) & 1]);
            next_enqueue = ia + 2;
        }
        HIP_CHECK(hipEventSynchronize(c->sweep_ev[ia & 1]));
        const double *res = c->pin_scal.p + RES_STRIDE * (ia & 1);
        const bool peer_failed = sl.shared_verdict && res[RES_VERD] != 0.0;
        if (peer_failed && !sl.fit_async) // cannot happen while the ranks are in lock-step (they enqueue the same form of fit)
            CGE_THROW(CGE_E_COLLECTIVE, "another rank abandoned a persistent fit this rank did not enqueue: the ranks diverged");
        if (sl.fit_async) {
            const int *hf = (const int *)(res + RES_FIT);
            if (hf[2] || !hf[0] || peer_failed) { // a wait timed out (here or on another rank): drain what was enqueued behind
                leave_persistent(c, directed, fit, sl);     // it and redo this alpha from its T_0 (still in place) with one
                next_enqueue = ia;                          // launch per iteration, as every later alpha
                ia--;
                continue;
            }
            sl.iters = hf[1];
            fit.prev_iters = sl.iters;
            c->stat_fit_persistent++;
            if (sl.fused) c->stat_fit_fused++;
        }
        c->stat_fit_iters += sl.iters;
        book.take(res, AlphaBook::AlphaStep * (double)ia, sl.iters);
        // cge_link_fit: this alpha has just become the best of the wanted kind -- its iterate is still where the slot says (the
        // next alpha, if already enqueued, reads it and writes another part of the ring; the one after is not enqueued yet;
        // directed sweeps are not enqueued ahead at all), so it is copied aside on the stream.  A redone alpha gets here once.
        if (c->link.cap_which) {
            const double a_now = AlphaBook::AlphaStep * (double)ia;
            if ((c->link.cap_which == CGE_LINK_BEST_LOCAL ? book.best_alpha_auc : book.best_alpha) == a_now)
                link_capture(c, sl.Ta, sl.Tb, N, sw.old2new, a_now);
        }
        if (book.ended()) break;
    }
    book.write(out, out_len);
    if (c->link.cap_which) { // what the model takes from the sweep besides the iterate: the diameter it normalised by, the power's form
        double lohi[2] = {0.0, orig ? orig->hi : 0.0};
        if (!orig) {
            HIP_CHECK(hipMemcpyAsync(lohi, c->sw_lohi.p, sizeof(lohi), hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        c->link.cap_hi = lohi[1];
        c->link.cap_pow = orig ? 0 : packed ? (c->opt_pow_exp2 ? 1 : 0) : (c->pow_logs_N == N ? 1 : 0);
    }
    c->stat_exact_packed = packed;
    if (!orig) { // the O(N^2) device storage this sweep required
        const i64 fpP = c->sweep_used_fp_P ? Nt64 * Nt64 * 64 * (i64)sizeof(double) * (directed ? 2 : 1) : 0;
        const i64 logs = c->pow_logs_N == N ? N * N * 12 : 0;
        c->stat_exact_matrix_bytes = packed ? Nt64 * (Nt64 + 1) / 2 * CGE_TILE_DOUBLES * (i64)sizeof(double) + fpP : 16 * N * N + logs + fpP;
    }
    if (c->stat_fit_persistent > 0 && !c->fit_persistent_broken) c->fit_fallback_streak = 0; // a clean persistent sweep
}

// ---- the alpha bookkeeping (common.hpp) ------------------------------------------------------------
AlphaBook::AlphaBook(i64 S_, int split_, cge_trace *trace_) : S(S_), split(split_), trace(trace_) {
    best_div = best_div_ext = best_div_int = best_auc_err = best_auc = INFINITY; // typemax(Float64)
    if (trace) trace->n_alpha = 0;
}

void AlphaBook::take(const double *res, double alpha, i64 iters) {
    double auc_val = NAN, div_val = NAN;
    if (!skip_auc) {
        double num = 0.0, den = 0.0;
        for (int b = 0; b < CGE_PARTIAL_BLOCKS; b++) { num += res[RES_AUC + 2 * b]; den += res[RES_AUC + 2 * b + 1]; }
        const double auc = 1.0 - num / den; // :213
        auc_val = auc;
        if (auc < best_auc) {
            best_auc = auc;
            best_auc_err = 1.96 * std::sqrt(auc * (1.0 - auc) / (double)S); // :217
            best_alpha_auc = alpha;
            auc_counter = 5;
        } else {
            auc_counter -= 1;
            skip_auc = auc_counter == 0;
        }
    }
    if (!skip_div) {
        double fa = 0.0, fb = 0.0; // all (or internal) / external
        for (int b = 0; b < CGE_PARTIAL_BLOCKS; b++) { fa += res[RES_JS + b]; fb += res[RES_JS + CGE_PARTIAL_BLOCKS + b]; }
        const double div_int = fa / 2.0, div_ext = fb / 2.0;
        const double f = !split ? fa / 2.0 : (div_int + div_ext) / 2.0;
        div_val = f;
        if (f < best_div) {
            best_div = f;
            best_alpha = alpha;
            best_div_ext = !split ? 0.0 : div_ext;
            best_div_int = !split ? 0.0 : div_int;
            div_counter = 5;
        } else {
            div_counter -= 1;
            skip_div = div_counter == 0;
        }
    }
    if (trace && trace->n_alpha < 64) {
        trace->iters[trace->n_alpha] = iters;
        trace->div[trace->n_alpha] = div_val;
        trace->auc[trace->n_alpha] = auc_val;
        trace->n_alpha++;
    }
}

void AlphaBook::write(double out[7], int *out_len) const {
    out[0] = best_alpha; out[1] = best_div; out[2] = best_div_ext; out[3] = best_div_int;
    out[4] = best_alpha_auc; out[5] = best_auc; out[6] = best_auc_err; // :256
    *out_len = 7;
}
