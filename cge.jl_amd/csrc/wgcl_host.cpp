// wgcl_host.cpp -- host side of the alpha sweep (wGCL / wGCL_directed, src/divergence.jl:27-257,
// :282-561) and the local-score sampler.  The host owns only the alpha bookkeeping (best/patience
// counters, :215-223, :242-253) and the batch-wise launch of fit iterations; every O(N^2) loop of the
// reference runs in kernels_fit.hip / kernels_dist.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "../../include/cge_hip_testing.h"

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
                        DevBuf<i32> &d_idx, DevBuf<i32> &d_out);

// full_graph_D of sampled vertex pairs (src/divergence.jl:104-114 restricted to the draws), dist()'s own arithmetic.  Option
// shard_rows: a pair's two rows may live on two ranks -- the rows of a chunk of pairs are gathered from their owners into a
// zero-filled buffer (all-reduce of the words: exact) and every rank evaluates the chunk from the gathered rows.
static void sampled_pair_dist(cge_ctx *c, const double *Xr, i64 d, const i32 *pi, const i32 *pj, i64 S, double den, double *out) {
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

// How a sweep lays its score graph out: the community -> members CSR, whether the graph is relabelled by community (the sweep's
// numbering) and whether the rest of an alpha's chain rides on the fit's launch (vect_B by tiles or not: c->bvec_blocks).
struct SweepLayout {
    std::vector<i32> cm_off, cm_mem; // community -> members, in the sweep's numbering
    bool relabel = false, fuse = false;
    i64 bt_total = 0;    // tile partials in all
    DevBuf<i32> old2new; // (relabel) a vertex's number in the sweep
};

// The layout decision from the communities alone (hcomm: 0-based, on the host): the community CSR, the tile tables (on the
// device when the tiles apply), c->bvec_blocks / c->bvec_contig and, for a relabelled sweep, the order (lay.cm_mem) and its
// inverse on the device.  landmarks: a landmark-mode sweep.  force_relabel: the testing hook's contiguous-row form below 8193
// vertices (every sweep passes false).  Shared by plan_layout and the testing hook cge_vect_b_test.
// packed_req: the sweep wants the packed form of its matrix, which goes with the tile form of vect_B at any N >= 256.
static void layout_tables(cge_ctx *c, const i32 *hcomm, i64 N, i64 C, int directed, bool landmarks, bool force_relabel,
                          SweepLayout &lay, bool packed_req = false) {
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
                          c->opt_pow_exp2 && flow_fused_applies(N);
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
static void plan_layout(cge_ctx *c, ScoreGraph &G, const OrigView *orig, int directed, SweepLayout &lay, bool packed_req,
                        bool force_relabel = false) {
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
static void community_tables(cge_ctx *c, const SweepLayout &lay, i64 N, i64 C, WordPacker &pk, std::vector<i32> &cm_pos) {
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
static i64 prepare_distances(cge_ctx *c, const ScoreGraph &G, const SweepLayout &lay, int directed, bool packed) {
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
static cge_fit_fused fused_entry(cge_ctx *c, const i32 *comm, i64 S, const double *dpos, const double *dneg, const double *wts) {
    cge_fit_fused e{};
    e.comm = comm; e.fc = c->sw_bt_fc.p; e.ns = c->sw_bt_ns.p; e.base = c->sw_bt_base.p; e.partial = c->sw_bt_part.p;
    e.S = S;
    e.dpos = dpos; e.dneg = dneg; e.wts = wts;
    e.auc_part = c->sw_scal.p + RES_AUC;
    return e;
}
// the tables' device copies (c->sw_fused_epi), which the fit's epilogue loads after its loop
static void fused_upload(cge_ctx *c, const std::vector<cge_fit_fused> &h_epi) {
    c->sw_fused_epi.ensure(h_epi.size() * sizeof(cge_fit_fused));
    static_assert(sizeof(cge_fit_fused) % 8 == 0, "packed as 4-byte words");
    WordPacker pk(c);
    pk.add(reinterpret_cast<i32 *>(c->sw_fused_epi.p), reinterpret_cast<const i32 *>(h_epi.data()),
           (i64)(h_epi.size() * sizeof(cge_fit_fused) / 4));
    pk.flush();
}
static void fused_tables(cge_ctx *c, const ScoreGraph &G, const OrigView *orig, const i32 *old2new, i64 n_sets, i64 s0, i64 s1,
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
    if (!flow_batch_member(N, device_cus(), false, &geo) || geo.G > h.max_G || !k_fit_flow_multi_fits(geo.NW, false)) return false;
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
    if (!flow_batch_member(N, device_cus(), true, &geo) || geo.G > h.max_G || !k_fit_flow_multi_fits(geo.NW, true)) return false;
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

// What the host keeps of an alpha in flight until it collects it (two at most: slot = alpha index mod 2)
struct AlphaSlot {
    bool fit_async = false;      // the fit was only enqueued: its verdict arrives with the alpha's scalars
    bool fused = false;          // the rest of the chain rode on the fit's launch
    bool shared_verdict = false; // N > 1, tallies split: the verdict of the fit travelled with the all-reduced tallies
    int t0_par = 0;              // the part of TT that held T_0 of this alpha
    i64 iters = 0;
};

// The form of the fit from alpha to alpha (a persistent form, once given up, stays given up for the sweep), the part of TT that
// holds the current iterate (undirected) and the last iteration count (the first batch of a launch-per-iteration fit).  eps,
// delta: the step and the stopping threshold -- a sweep's are the reference's (0.25 undirected :119, 0.9 directed :434; delta
// :35); the testing hook cge_fit_test passes its caller's.
struct FitForm {
    bool persistent = false, persistent_dir = false;
    int tpar = 0;
    i64 prev_iters = 16;
    double eps = 0.25, delta = AlphaBook::delta;
};

// Whether a sweep starts on the persistent form of its fit (the geometry is asked at the first launch)
static bool persistent_wanted(const cge_ctx *c, i64 N) {
    return !c->fit_persistent_broken && c->opt_fit_persistent != 1 && (c->opt_fit_persistent >= 2 || N >= 128);
}

// One launch (pair) per iteration: `launch(k)` enqueues iteration k, in batches -- the first as long as the previous fit, at
// most 32 from then on.  After each batch the host reads the fit's flags ([0] done, [1] iterations) and, when `ring` is given,
// the changes of the undirected fit's last iterations.  Returns the iterations.
template <class Launch>
static i64 fit_by_launches(cge_ctx *c, i64 prev_iters, double alpha, double delta, const int *flags,
                           const unsigned long long *ring, Launch launch) {
    hipStream_t st = c->stream;
    i64 batch = std::max<i64>(4, std::min<i64>(prev_iters, 128));
    for (i64 k = 0;;) {
        for (i64 b = 0; b < batch; b++, k++) launch(k);
        int hf[2];
        unsigned long long hr[3];
        HIP_CHECK(hipMemcpyAsync(hf, flags, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
        if (ring) HIP_CHECK(hipMemcpyAsync(hr, ring, sizeof(hr), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const i64 iters = hf[1];
        if (hf[0]) return iters;
        if (ring) {
            double flast;
            std::memcpy(&flast, &hr[(k - 1) % 3], sizeof(double));
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
static void fit_undirected(cge_ctx *c, i64 N, const double *w, i64 Tld, double alpha, bool upper, bool packed,
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
static void fit_directed(cge_ctx *c, const ScoreGraph &G, double alpha, FitForm &fit, AlphaSlot &sl) {
    hipStream_t st = c->stream;
    const i64 N = G.N;
    const double *GD = c->sw_GD.p;
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
    sl.iters = fit_by_launches(c, fit.prev_iters, alpha, fit.delta, flags, nullptr, [&](i64) {
        k_fit_symv_dir(c, GD, Tin, Tout, N, c->sw_S1.p, c->sw_S2.p, flags);
        k_fit_update_dir(c, Tin, Tout, c->sw_S1.p, c->sw_S2.p, G.deg_in, G.deg_out, N, fit.delta, flags, flags + 1,
                         c->sw_fitstate.p);
    });
}

// An enqueued persistent fit was abandoned: what was enqueued behind it is drained, and this fit and every later one of the
// sweep go by one launch per iteration -- this one again from its T_0, which is still in place.
static void leave_persistent(cge_ctx *c, int directed, FitForm &fit, const AlphaSlot &sl) {
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
    if (packed && want_div && !(c->bvec_blocks && !directed && !c->opt_test_bvec_plain))
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
            else k_bvec(c, GD, Ta, Tb, c->sw_cm_pos.p, cm_off, c->sw_cm_mem.p, N, C, directed, c->sw_rowbins.p, vectB);
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
static void packed_buffers(cge_ctx *c, i64 N) {
    const i64 Nt = (N + 63) / 64, NT = Nt * (Nt + 1) / 2;
    const size_t pk_words = (size_t)NT * CGE_TILE_DOUBLES, fp_words = (size_t)Nt * Nt * 64;
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
    // layout), option "exact_packed" = 1 wherever it applies.  Directed sweeps stay resident, with the limit.
    const double resident_limit = c->opt_test_resident_limit > 0 ? c->opt_test_resident_limit : 200e9;
    const bool beyond = (double)N * (double)N * 8.0 * 2.2 > resident_limit;
    const bool packed_req = !orig && !directed && (beyond || c->opt_exact_packed == 1);
    c->stat_exact_packed = 0;
    if (beyond && !packed_req) CGE_THROW(CGE_E_OOM, "score graph with %lld vertices does not fit", (long long)N);
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
    if (packed) packed_buffers(c, N);
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
    fit.persistent_dir = directed && persistent_wanted(c, N);
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
        if (book.ended()) break;
    }
    book.write(out, out_len);
    c->stat_exact_packed = packed;
    if (!orig) { // the O(N^2) device storage this sweep required
        const i64 fpP = c->sweep_used_fp_P ? Nt64 * Nt64 * 64 * (i64)sizeof(double) : 0;
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


// ---- the testing hook of vect_B (include/cge_hip_testing.h: cge_vect_b_test) ------------------------------------------

namespace {
struct VbOptions { // the two options that choose vect_B's form, as the hook sets them for a forced form; restored on the way out
    cge_ctx *c;
    int blocks, plain;
    explicit VbOptions(cge_ctx *c_) : c(c_), blocks(c_->opt_bvec_blocks), plain(c_->opt_test_bvec_plain) {}
    ~VbOptions() { c->opt_bvec_blocks = blocks; c->opt_test_bvec_plain = plain; }
};
} // namespace

static i64 vb_len(i64 C, int directed) { return directed ? C * C : packed_len(C); }

// One problem as a sweep lays it out -- layout_tables, the host arrays permuted by its order (the sweep computes GD from permuted
// rows), GD / Ta / Tb in sw_GD / sw_T1 / sw_T2, community_tables, k_bins_prepare -- after the checks of a forced form, which
// come before anything is launched.  Returns the form to run.
static int vb_prepare(cge_ctx *c, const cge_vect_b_problem &p, int directed, int form, bool landmarks) {
    const i64 N = p.N, C = p.C;
    if (form == 1 && N * sizeof(double) > 64 * 1024)
        CGE_THROW(CGE_E_ARG, "vect_b_test: a row of %lld vertices does not fit the LDS of the staged row bins", (long long)N);
    if (form >= 4 && (N < 256 || C < 2))
        CGE_THROW(CGE_E_ARG, "vect_b_test: the tiles need 256 vertices and 2 communities (N = %lld, C = %lld)", (long long)N, (long long)C);
    if (form == 2) c->opt_test_bvec_plain = 1;
    else if (form != 0) { c->opt_test_bvec_plain = 0; c->opt_bvec_blocks = form >= 4; }
    std::vector<i32> hcomm(N);
    for (i64 i = 0; i < N; i++) {
        if (p.comm[i] < 1 || p.comm[i] > C) CGE_THROW(CGE_E_ARG, "vect_b_test: community id out of range");
        hcomm[i] = (i32)(p.comm[i] - 1);
    }
    SweepLayout lay;
    layout_tables(c, hcomm.data(), N, C, directed, form == 0 && landmarks, form == 3, lay);
    if (form >= 4 && !c->bvec_blocks)
        CGE_THROW(CGE_E_ARG, "vect_b_test: the tiles decline this layout (more than 64 community ids in a 64-vertex block)");
    const int run = form != 0 ? form : (c->bvec_blocks && !directed && !c->opt_test_bvec_plain) ? 5 : k_bvec_form(c, N);
    hipStream_t st = c->stream;
    c->sw_GD.ensure((size_t)N * N);
    c->sw_T1.ensure(N); c->sw_T2.ensure(N);
    c->sw_rowbins.ensure((size_t)N * C);
    std::vector<double> hGD, hTa, hTb; // (relabelled) in the sweep's numbering
    if (lay.relabel) {
        const std::vector<i32> order = lay.cm_mem;
        hGD.resize((size_t)N * N); hTa.resize(N); hTb.resize(N);
        for (i64 q = 0; q < N; q++) {
            const i64 a = order[q];
            hTa[q] = p.Ta[a]; hTb[q] = p.Tb[a];
            double *dst = hGD.data() + q * N;
            if (directed)
                for (i64 r = 0; r < N; r++) dst[r] = p.GD[a * N + order[r]];
            else // the caller's upper triangle is the matrix
                for (i64 r = 0; r < N; r++) {
                    const i64 b = order[r];
                    dst[r] = a <= b ? p.GD[a * N + b] : p.GD[b * N + a];
                }
        }
        for (i64 q = 0; q < N; q++) lay.cm_mem[q] = (i32)q; // the member lists in the new numbering, as plan_layout leaves them
    }
    HIP_CHECK(hipMemcpyAsync(c->sw_GD.p, lay.relabel ? hGD.data() : p.GD, sizeof(double) * N * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->sw_T1.p, lay.relabel ? hTa.data() : p.Ta, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->sw_T2.p, lay.relabel ? hTb.data() : p.Tb, sizeof(double) * N, hipMemcpyHostToDevice, st));
    WordPacker pk(c);
    std::vector<i32> cm_pos;
    community_tables(c, lay, N, C, pk, cm_pos);
    pk.flush();
    if (c->bvec_blocks && !directed) k_bins_prepare(c, c->sw_cm_off.p, N, C, lay.bt_total);
    HIP_CHECK(hipStreamSynchronize(st)); // (the host copies go out of scope)
    return run;
}

// the block partials of a divergence added in block order, then halved: what AlphaBook::take and js_final_kernel do
static double vb_fold(const double *fpart) {
    double f = 0.0;
    for (int b = 0; b < CGE_PARTIAL_BLOCKS; b++) f += fpart[b];
    return f / 2.0;
}

void host_vect_b_test(cge_ctx *c, const cge_vect_b_problem *p1, const cge_vect_b_problem *p2, int directed, int form,
                      int landmarks, int n_modes, int *form_ran) {
    const cge_vect_b_problem *probs[2] = {p1, form == 6 ? p2 : nullptr};
    if ((form == 5 || form == 6) && directed) CGE_THROW(CGE_E_ARG, "vect_b_test: form %d is undirected only", form);
    if (form == 6 && (!p2 || !p2->GD || p2->C >= p1->C)) CGE_THROW(CGE_E_ARG, "vect_b_test: form 6 takes a second problem of fewer communities");
    for (const cge_vect_b_problem *p : probs) {
        if (!p) continue;
        if (p->N <= 0 || p->C <= 0 || !p->vectB) CGE_THROW(CGE_E_ARG, "vect_b_test: empty problem");
        if (p->GD && (!p->Ta || !p->Tb || !p->comm)) CGE_THROW(CGE_E_ARG, "vect_b_test: Ta, Tb and comm go with GD");
        if (p->vC && !p->js_dev) CGE_THROW(CGE_E_ARG, "vect_b_test: vC without js_dev");
        if ((double)p->N * (double)p->C > 1e9) CGE_THROW(CGE_E_ARG, "vect_b_test: problem too large");
    }
    if (!p1->GD && (!p1->vC || form != 0)) CGE_THROW(CGE_E_ARG, "vect_b_test: the JS-only mode takes vC, vectB and form 0");
    hipStream_t st = c->stream;
    VbOptions restore(c);
    const i64 G = CGE_VECT_B_GUARD;
    const i64 len[2] = {vb_len(p1->C, directed), probs[1] ? vb_len(probs[1]->C, directed) : 0};
    const i64 off[2] = {0, len[0] + G};
    // both vectors back to back, each followed by a guard of NaNs that nothing may write
    std::vector<double> hv((size_t)(len[0] + len[1] + 2 * G), std::nan(""));
    if (!p1->GD) std::memcpy(hv.data(), p1->vectB, sizeof(double) * len[0]);
    DevBuf<double> vB, vC, fpart, part, jsd;
    vB.ensure(hv.size());
    HIP_CHECK(hipMemcpyAsync(vB.p, hv.data(), sizeof(double) * hv.size(), hipMemcpyHostToDevice, st));
    { // vect_C of both problems (zeros where the caller has none and the form reads one)
        std::vector<double> hc((size_t)(len[0] + len[1]), 0.0);
        for (int q = 0; q < 2; q++)
            if (probs[q] && probs[q]->vC) std::memcpy(hc.data() + (q ? len[0] : 0), probs[q]->vC, sizeof(double) * len[q]);
        vC.ensure(hc.size());
        HIP_CHECK(hipMemcpyAsync(vC.p, hc.data(), sizeof(double) * hc.size(), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    const double *vCp[2] = {vC.p, vC.p + len[0]};
    const int nm = n_modes == 2 ? 2 : 1;
    fpart.ensure((size_t)4 * CGE_PARTIAL_BLOCKS);
    int run = 0;
    if (p1->GD && form != 6) {
        run = vb_prepare(c, *p1, directed, form, landmarks != 0);
        const i64 N = p1->N, C = p1->C;
        if (run == 5) {
            k_bvec_tiles(c, c->sw_GD.p, c->sw_T1.p, c->sw_T2.p, c->sw_cm_off.p, N, directed);
            k_bins_js(c, c->sw_cm_off.p, N, C, vCp[0], vB.p, nm, fpart.p);
        } else
            k_bvec(c, c->sw_GD.p, c->sw_T1.p, c->sw_T2.p, c->sw_cm_pos.p, c->sw_cm_off.p, c->sw_cm_mem.p, N, C, directed,
                   c->sw_rowbins.p, vB.p, run);
    } else if (p1->GD) { // form 6: the tile partials of the first problem leave the context, as a batch member's do
        run = 6;
        DevBuf<i32> fc1, ns1, base1, off1;
        DevBuf<double> part1;
        vb_prepare(c, *p1, 0, 6, false);
        k_bvec_tiles(c, c->sw_GD.p, c->sw_T1.p, c->sw_T2.p, c->sw_cm_off.p, p1->N, 0);
        HIP_CHECK(hipStreamSynchronize(st));
        fc1.swap(c->sw_bt_fc); ns1.swap(c->sw_bt_ns); base1.swap(c->sw_bt_base); part1.swap(c->sw_bt_part); off1.swap(c->sw_cm_off);
        vb_prepare(c, *p2, 0, 6, false);
        k_bvec_tiles(c, c->sw_GD.p, c->sw_T1.p, c->sw_T2.p, c->sw_cm_off.p, p2->N, 0);
        cge_bins_multi bins{};
        cge_js_multi js{};
        bins.p[0] = cge_bins_problem{part1.p, off1.p, fc1.p, ns1.p, base1.p, p1->C, (int)((p1->N + 63) / 64), 0, vB.p + off[0]};
        bins.p[1] = cge_bins_problem{c->sw_bt_part.p, c->sw_cm_off.p, c->sw_bt_fc.p, c->sw_bt_ns.p, c->sw_bt_base.p, p2->C,
                                     (int)((p2->N + 63) / 64), 0, vB.p + off[1]};
        part.ensure((size_t)4 * 3 * CGE_PARTIAL_BLOCKS);
        int nj = 0;
        for (int q = 0; q < 2; q++)
            for (int u = 0; u < nm; u++, nj++)
                js.p[nj] = cge_js_problem{vCp[q], vB.p + off[q], len[q], probs[q]->C, nm == 1 ? 0 : 1 + u, 0,
                                          part.p + (i64)nj * 3 * CGE_PARTIAL_BLOCKS, fpart.p + (i64)nj * CGE_PARTIAL_BLOCKS};
        k_bins_js_multi(c, bins, 2, p1->C, js, nj);
        HIP_CHECK(hipStreamSynchronize(st)); // (the first problem's tables are released below)
    }
    *form_ran = run;
    std::vector<double> hf((size_t)4 * CGE_PARTIAL_BLOCKS, 0.0);
    if (run >= 5) HIP_CHECK(hipMemcpyAsync(hf.data(), fpart.p, sizeof(double) * hf.size(), hipMemcpyDeviceToHost, st));
    // k_js modes 0, 1, 2 over the vector(s) the form left
    jsd.ensure(6);
    double hj[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 2; q++)
        if (probs[q] && probs[q]->vC)
            for (int mode = 0; mode < 3; mode++)
                k_js(c, vCp[q], vB.p + off[q], len[q], probs[q]->C, directed, mode, jsd.p + 3 * q + mode);
    HIP_CHECK(hipMemcpyAsync(hj, jsd.p, sizeof(hj), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hv.data(), vB.p, sizeof(double) * hv.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int q = 0; q < 2; q++) {
        const cge_vect_b_problem *p = probs[q];
        if (!p) continue;
        if (p->GD) std::memcpy(p->vectB, hv.data() + off[q], sizeof(double) * (len[q] + G));
        if (p->vC) std::memcpy(p->js_dev, hj + 3 * q, sizeof(double) * 3);
        if (p->js_fused && run >= 5)
            for (int u = 0; u < nm; u++) p->js_fused[u] = vb_fold(hf.data() + (i64)((run == 6 ? q * nm : 0) + u) * CGE_PARTIAL_BLOCKS);
    }
}

// ---- the testing hook of the Chung-Lu fit (include/cge_hip_testing.h: cge_fit_test) -------------------------------------------
// One fit from a caller's start through fit_undirected / fit_directed (forms 0-4), k_fit_flow_multi (form 5) or
// k_fit_flow_dir_multi (form 6), on the buffers a sweep keeps them in.  Everything that can refuse does so before the first launch.

// D to sw_D and, when the form or the caller reads it, GD = (1 - D)^alpha to sw_GD by the sweep's two launches (upper: the upper
// tiles alone, as a landmark-mode sweep makes it; everything else of sw_GD is NaN) and to the caller's GD
static void ft_matrices(cge_ctx *c, const cge_fit_problem &p, bool upper, bool need_gd) {
    hipStream_t st = c->stream;
    const i64 N = p.N;
    c->sw_D.ensure((size_t)N * N);
    HIP_CHECK(hipMemcpyAsync(c->sw_D.p, p.D, sizeof(double) * N * N, hipMemcpyHostToDevice, st));
    if (need_gd || p.GD) {
        c->sw_GD.ensure((size_t)N * N);
        HIP_CHECK(hipMemsetAsync(c->sw_GD.p, 0xFF, sizeof(double) * N * N, st)); // (all bits set: a NaN)
        k_pow_prepare(c, c->sw_D.p, N, upper);
        k_pow_matrix(c, c->sw_D.p, N, p.alpha, c->sw_GD.p, upper);
        if (p.GD) HIP_CHECK(hipMemcpyAsync(p.GD, c->sw_GD.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

// the verdict of an enqueued persistent fit: flags [0] converged, [1] iterations, [2] abandoned
static bool ft_verdict(cge_ctx *c, const int *dev_flags, i64 *iters) {
    int hf[4];
    HIP_CHECK(hipMemcpyAsync(hf, dev_flags, sizeof(hf), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    *iters = hf[1];
    return !(hf[2] || !hf[0]);
}

// epi / epi_dev (form 4, the hooks of the local score and of the fused chain): the host and device copies of the epilogue's table
// (fused_tables); the launch then wants of the epilogue what epi_want names (bit 0 vect_B's tile partials, bit 1 the tally), as
// enqueue_alpha leaves out what an alpha does not want -- the local score's hook the tally alone.
static int ft_undirected(cge_ctx *c, cge_fit_problem &p, int form, double eps, double delta, const cge_fit_fused *epi = nullptr,
                         const cge_fit_fused *epi_dev = nullptr, int epi_want = 2) {
    hipStream_t st = c->stream;
    const i64 N = p.N, Nt = (N + 63) / 64, Tld = Nt * 64;
    ft_matrices(c, p, true, form != 4);
    if (form == 2) { // the upper tiles of GD, zeros outside the matrix, through the address inline every consumer uses
        std::vector<double> h((size_t)N * N), pk((size_t)(Nt * (Nt + 1) / 2) * CGE_TILE_DOUBLES, 0.0);
        HIP_CHECK(hipMemcpyAsync(h.data(), c->sw_GD.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (i64 i = 0; i < N; i++)
            for (i64 j = i / 64 * 64; j < N; j++) pk[cge_packed_index(i, j, Nt)] = h[i * N + j];
        c->sw_PK.ensure(pk.size());
        HIP_CHECK(hipMemcpyAsync(c->sw_PK.p, pk.data(), sizeof(double) * pk.size(), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (form == 4) k_pow_prepare(c, c->sw_D.p, N, true, true);
    // T_0 in part 0 of TT (zero beyond N), NaN in the rows of the two other parts
    DevBuf<double> dw;
    dw.ensure(N);
    c->fp_T.ensure((size_t)3 * Tld);
    c->sw_scal.ensure(RES_STRIDE);
    c->sw_flags.ensure(4);
    c->sw_fring.ensure(4);
    const std::vector<double> nan_n(N, std::nan(""));
    HIP_CHECK(hipMemsetAsync(c->fp_T.p, 0, sizeof(double) * 3 * Tld, st));
    HIP_CHECK(hipMemcpyAsync(c->fp_T.p, p.T0, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->fp_T.p + Tld, nan_n.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->fp_T.p + 2 * Tld, nan_n.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dw.p, p.w, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    c->flow_armed_words = 0; // (no alpha of a sweep armed the hand-off slots of this launch)
    FitForm fit;
    fit.eps = eps;
    fit.delta = delta;
    fit.persistent = form == 3 || form == 4 || (form == 0 && persistent_wanted(c, N));
    cge_fit_fused ff{};
    if (epi) { // (else no partial, no auc_part: nothing is wanted of the epilogue)
        ff = *epi;
        if (!(epi_want & 1)) ff.partial = nullptr;
        if (!(epi_want & 2)) ff.auc_part = nullptr;
    }
    ff.Lh = c->sw_Lh.p; ff.Ll = c->sw_Ll.p; ff.alpha = p.alpha;
    AlphaSlot sl;
    fit_undirected(c, N, dw.p, Tld, p.alpha, true, form == 2, form == 4 ? &ff : nullptr, form == 4 ? epi_dev : nullptr, fit, sl);
    int ran = form == 2 ? 2 : 1;
    p.status = 0;
    if (sl.fit_async) {
        ran = form == 4 ? 4 : 3;
        if (!ft_verdict(c, (const int *)(c->sw_scal.p + RES_FIT), &sl.iters)) {
            if (form == 0) { // as the sweep: again from T_0 with one launch pair per iteration
                leave_persistent(c, 0, fit, sl);
                sl = AlphaSlot();
                fit_undirected(c, N, dw.p, Tld, p.alpha, true, false, nullptr, nullptr, fit, sl);
                ran = 1;
            } else
                p.status = 1;
        }
    } else if (form == 3 || form == 4)
        CGE_THROW(CGE_E_ASSERT, "fit_test: the persistent launch of form %d was declined (N = %lld)", form, (long long)N);
    p.iters = sl.iters;
    HIP_CHECK(hipMemcpyAsync(p.T, c->fp_T.p + (i64)fit.tpar * Tld, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (form == 2) c->sw_PK.release(); // (held only while packed sweeps run)
    return ran;
}

static int ft_directed(cge_ctx *c, cge_fit_problem &p, int form, double eps, double delta) {
    hipStream_t st = c->stream;
    const i64 N = p.N;
    ft_matrices(c, p, false, true);
    DevBuf<double> din, dout;
    din.ensure(N); dout.ensure(N);
    c->sw_T1.ensure(N); c->sw_T2.ensure(N); c->sw_S1.ensure(N); c->sw_S2.ensure(N);
    c->sw_scal.ensure(RES_STRIDE);
    c->sw_flags.ensure(4);
    c->sw_fitstate.ensure(4);
    HIP_CHECK(hipMemcpyAsync(c->sw_T1.p, p.T0, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->sw_T2.p, p.T0b, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(din.p, p.w, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dout.p, p.w2, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ScoreGraph G;
    G.N = N;
    G.deg_in = din.p; G.deg_out = dout.p;
    FitForm fit;
    fit.eps = eps;
    fit.delta = delta;
    fit.persistent_dir = form == 3 || (form == 0 && persistent_wanted(c, N));
    AlphaSlot sl;
    fit_directed(c, G, p.alpha, fit, sl);
    int ran = 1;
    p.status = 0;
    if (sl.fit_async) {
        ran = 3;
        if (!ft_verdict(c, (const int *)(c->sw_scal.p + RES_FIT), &sl.iters)) {
            if (form == 0) {
                leave_persistent(c, 1, fit, sl);
                sl = AlphaSlot();
                fit_directed(c, G, p.alpha, fit, sl);
                ran = 1;
            } else
                p.status = 1;
        }
    } else if (form == 3)
        CGE_THROW(CGE_E_ASSERT, "fit_test: the persistent launch of form 3 was declined (N = %lld)", (long long)N);
    p.iters = sl.iters;
    HIP_CHECK(hipMemcpyAsync(p.T, c->sw_T1.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(p.Tb, c->sw_T2.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return ran;
}

// A member of a shared undirected launch with its own logarithm, T and weights, as the members of a batch keep them
// (batch_host.cpp), and its entry of the launch's table: T_0 (zero beyond N), then the result (NaN until written)
struct FtMember {
    DevBuf<double> Lh, T, w;
    DevBuf<float> Ll;
};
static cge_flow_problem ft_member(cge_ctx *c, const cge_fit_problem &p, const FlowGeometry &geo, FtMember &m, int *flags,
                                  const cge_fit_fused *epi, int want) {
    hipStream_t st = c->stream;
    const i64 N = p.N, Tld = (i64)geo.Nt * 64;
    ft_matrices(c, p, true, false);
    k_pow_prepare(c, c->sw_D.p, N, true, true);
    HIP_CHECK(hipStreamSynchronize(st));
    m.Lh.swap(c->sw_Lh); m.Ll.swap(c->sw_Ll);
    c->pow_logs_N = c->pow_logs_blocked_N = 0; // (the context's logarithm left with the member)
    m.T.ensure((size_t)2 * Tld);
    m.w.ensure(N);
    const std::vector<double> nan_n(N, std::nan(""));
    HIP_CHECK(hipMemsetAsync(m.T.p, 0, sizeof(double) * 2 * Tld, st));
    HIP_CHECK(hipMemcpyAsync(m.T.p, p.T0, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.T.p + Tld, nan_n.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.w.p, p.w, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return flow_problem_entry(m.Lh.p, m.Ll.p, p.alpha, epi, want, m.T.p, m.T.p + Tld, m.w.p, flags, N, Tld, geo);
}
// the members' verdicts and iterates of a shared launch
static void ft_multi_collect(cge_ctx *c, cge_fit_problem *probs, int n, const cge_flow_multi &tab) {
    for (int i = 0; i < n; i++) {
        cge_fit_problem &p = probs[i];
        p.status = ft_verdict(c, tab.p[i].flags, &p.iters) ? 0 : 1;
        HIP_CHECK(hipMemcpyAsync(p.T, tab.p[i].Tout, sizeof(double) * p.N, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// form 5: every problem with slots and flags of its own; nothing is wanted of the epilogue
static void ft_multi(cge_ctx *c, cge_fit_problem *probs, int n, const FlowGeometry *geo, double eps, double delta) {
    hipStream_t st = c->stream;
    std::vector<std::unique_ptr<FtMember>> mem;
    DevBuf<int> flags;
    DevBuf<double> flow;
    flags.ensure((size_t)4 * n);
    HIP_CHECK(hipMemsetAsync(flags.p, 0, sizeof(int) * 4 * n, st));
    cge_flow_multi tab{};
    tab.n = n;
    for (int i = 0; i < n; i++) {
        mem.emplace_back(new FtMember());
        tab.p[i] = ft_member(c, probs[i], geo[i], *mem.back(), flags.p + 4 * i, nullptr, 0);
    }
    k_fit_flow_multi(c, tab, geo[0].NW, eps, delta, flow);
    ft_multi_collect(c, probs, n, tab);
}

// form 6: every problem with its own power matrix, Tin / Tout, degrees and flags, as the directed members of a batch keep them
static void ft_dir_multi(cge_ctx *c, cge_fit_problem *probs, int n, const FlowGeometry *geo, double eps, double delta) {
    hipStream_t st = c->stream;
    struct Member {
        DevBuf<double> GD, T, deg;
    };
    std::vector<std::unique_ptr<Member>> mem;
    DevBuf<int> flags;
    DevBuf<double> flow;
    flags.ensure((size_t)4 * n);
    HIP_CHECK(hipMemsetAsync(flags.p, 0, sizeof(int) * 4 * n, st));
    cge_flow_dir_multi tab{};
    tab.n = n;
    for (int i = 0; i < n; i++) {
        cge_fit_problem &p = probs[i];
        const i64 N = p.N, Tld = (i64)geo[i].Nt * 64;
        mem.emplace_back(new Member());
        Member &m = *mem.back();
        ft_matrices(c, p, false, true);
        m.GD.swap(c->sw_GD); // (the context's power matrix leaves with the member)
        m.T.ensure((size_t)2 * N);
        m.deg.ensure((size_t)2 * N);
        HIP_CHECK(hipMemcpyAsync(m.T.p, p.T0, sizeof(double) * N, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(m.T.p + N, p.T0b, sizeof(double) * N, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(m.deg.p, p.w, sizeof(double) * N, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(m.deg.p + N, p.w2, sizeof(double) * N, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        cge_flow_dir_problem &q = tab.p[i];
        q.GD = m.GD.p;
        q.Tin = m.T.p; q.Tout = m.T.p + N;
        q.deg_in = m.deg.p; q.deg_out = m.deg.p + N;
        q.flags = flags.p + 4 * i;
        q.N = N; q.Tld = Tld; q.Nt = geo[i].Nt; q.G = geo[i].G;
    }
    k_fit_flow_dir_multi(c, tab, geo[0].NW, eps, 1.0, delta, flow);
    for (int i = 0; i < n; i++) {
        cge_fit_problem &p = probs[i];
        p.status = ft_verdict(c, flags.p + 4 * i, &p.iters) ? 0 : 1;
        HIP_CHECK(hipMemcpyAsync(p.T, tab.p[i].Tin, sizeof(double) * p.N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(p.Tb, tab.p[i].Tout, sizeof(double) * p.N, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

void host_fit_test(cge_ctx *c, cge_fit_problem *probs, int n, int directed, int form, double eps, double delta, int *form_ran) {
    if (!directed && form == 6) CGE_THROW(CGE_E_ARG, "fit_test: form 6 is directed only");
    if (n > 1 && form != 5 && form != 6) CGE_THROW(CGE_E_ARG, "fit_test: %d problems in one call are form 5 only", n);
    if (n > CGE_BATCH_MAX) CGE_THROW(CGE_E_ARG, "fit_test: form %d takes at most %d problems", form, CGE_BATCH_MAX);
    if (directed && (form == 2 || form == 4 || form == 5)) CGE_THROW(CGE_E_ARG, "fit_test: form %d is undirected only", form);
    if ((form == 4 || form == 5) && !c->opt_pow_exp2)
        CGE_THROW(CGE_E_ARG, "fit_test: form %d makes its power matrix from the stored logarithm (option pow_exp2)", form);
    if (!(eps > 0.0) || !(delta >= 0.0)) CGE_THROW(CGE_E_ARG, "fit_test: eps > 0 and delta >= 0");
    const bool multi = form == 5 || form == 6;
    FlowGeometry geo[CGE_BATCH_MAX];
    int sumG = 0;
    const int cus = device_cus();
    for (int i = 0; i < n; i++) {
        const cge_fit_problem &p = probs[i];
        if (p.N <= 0 || !p.D || !p.w || !p.T0 || !p.T) CGE_THROW(CGE_E_ARG, "fit_test: empty problem");
        if (directed && (!p.w2 || !p.T0b || !p.Tb)) CGE_THROW(CGE_E_ARG, "fit_test: a directed problem takes w2, T0b and Tb");
        if (p.N > 46340) CGE_THROW(CGE_E_ARG, "fit_test: problem too large");
        FlowGeometry &g = geo[i];
        const bool applies = flow_geometry(p.N, cus, &g);
        if (form == 3 && !applies)
            CGE_THROW(CGE_E_ARG, "fit_test: the geometry of the persistent fit declines N = %lld on %d CUs", (long long)p.N, cus);
        if ((form == 4 || form == 5) && !(applies && g.fused()))
            CGE_THROW(CGE_E_ARG, "fit_test: the geometry of the fused persistent fit declines N = %lld on %d CUs", (long long)p.N, cus);
        if (!multi) continue;
        if (!applies)
            CGE_THROW(CGE_E_ARG, "fit_test: the geometry of the directed persistent fit declines N = %lld on %d CUs", (long long)p.N, cus);
        if (!g.fused())
            CGE_THROW(CGE_E_ARG, "fit_test: form 6 takes problems of one quarter block per workgroup (N = %lld needs two on %d CUs)", (long long)p.N, cus);
        if (g.NW != geo[0].NW)
            CGE_THROW(CGE_E_ARG, "fit_test: form %d takes problems of one NW (problem %d runs %d waves per workgroup, problem 0 runs %d)", form, i, g.NW, geo[0].NW);
        sumG += g.G;
    }
    if (!multi) {
        *form_ran = directed ? ft_directed(c, probs[0], form, eps, delta) : ft_undirected(c, probs[0], form, eps, delta);
        return;
    }
    if (sumG > cus)
        CGE_THROW(CGE_E_ARG, "fit_test: the problems of form %d need %d workgroups in all, the device has %d CUs", form, sumG, cus);
    if (!k_fit_flow_multi_fits(geo[0].NW, form == 6))
        CGE_THROW(CGE_E_ARG, "fit_test: %s of %d waves gets no workgroup on a CU", form == 6 ? "fit_flow_dir_multi_kernel" : "fit_flow_multi_kernel",
                  geo[0].NW);
    (form == 6 ? ft_dir_multi : ft_multi)(c, probs, n, geo, eps, delta);
    *form_ran = form;
}

// host <-> device copies of the hooks below on the context's stream (down: a NULL host pointer is not copied)
template <class T>
static void ls_up(cge_ctx *c, DevBuf<T> &dev, const T *host, i64 cnt) {
    dev.ensure((size_t)cnt);
    HIP_CHECK(hipMemcpyAsync(dev.p, host, sizeof(T) * cnt, hipMemcpyHostToDevice, c->stream));
}
template <class T>
static void ls_down(cge_ctx *c, T *host, const T *dev, i64 cnt) {
    if (host) HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(T) * cnt, hipMemcpyDeviceToHost, c->stream));
}

// ---- the testing hook of the fused chain (include/cge_hip_testing.h: cge_fused_chain_test) -----------------------------------
// One alpha as enqueue_alpha / host_batch_sweep run it on the fused path, on a caller's problem: the layout and its tables, the
// epilogue's table, the fit with its epilogue's outputs wanted, the bins and the divergence.  A problem is prepared on the
// context's buffers, as a sweep prepares it; the problems of a shared launch then take them along (FcMember), as hand_off does.
namespace {
struct FcOptions { // the options that decide whether a layout is the fused one, as the hook sets them; restored on the way out
    cge_ctx *c;
    int fused, plain, persistent;
    bool relabel;
    explicit FcOptions(cge_ctx *c_)
        : c(c_), fused(c_->opt_fit_fused), plain(c_->opt_test_bvec_plain), persistent(c_->opt_fit_persistent), relabel(c_->opt_exact_relabel) {}
    ~FcOptions() { c->opt_fit_fused = fused; c->opt_test_bvec_plain = plain; c->opt_fit_persistent = persistent; c->opt_exact_relabel = relabel; }
};
struct FcMember {
    std::vector<i32> order;                  // the layout's order: the caller's vertex at each position of the sweep's numbering
    std::vector<double> D, w, T0, T;         // the problem in the sweep's numbering
    i64 bt_total = 0, vlen = 0;
    cge_fit_fused epi{};                     // the host copy of the epilogue's table
    DevBuf<i32> comm, aidx, fc, ns, base, cm_off; // (fc .. cm_off: a shared launch's members take the context's along)
    DevBuf<double> afac, dpos, dneg, wts, apw, part, scal, vB, vC, fpart, jspart;
    DevBuf<char> epi_dev;
    FtMember fit;
};
} // namespace

// The layout, the tables and the epilogue's table of one problem, on the context.  Every refusal of the layout comes first.
static void fc_prepare(cge_ctx *c, const cge_fused_chain_problem &p, FcMember &m, bool shared) {
    hipStream_t st = c->stream;
    const i64 N = p.N, C = p.C, Nt = (N + 63) / 64, S = (p.want & 2) ? p.S : 0;
    std::vector<i32> hcomm(N);
    for (i64 i = 0; i < N; i++) {
        if (p.comm[i] < 1 || p.comm[i] > C) CGE_THROW(CGE_E_ARG, "fused_chain_test: community id out of range");
        hcomm[i] = (i32)(p.comm[i] - 1);
    }
    SweepLayout lay;
    layout_tables(c, hcomm.data(), N, C, 0, true, false, lay);
    if (!c->bvec_blocks)
        CGE_THROW(CGE_E_ARG, "fused_chain_test: the tiles decline this layout (more than 64 community ids in a 64-vertex block)");
    if (!lay.fuse)
        CGE_THROW(CGE_E_ARG, "fused_chain_test: the fused form declines this layout (more than %d pieces in a 64-vertex block)", CGE_FLOW_NP);
    if (p.partials && p.partials_cap < lay.bt_total)
        CGE_THROW(CGE_E_ARG, "fused_chain_test: partials holds %lld doubles, the layout has %lld tile partials", (long long)p.partials_cap,
                  (long long)lay.bt_total);
    m.bt_total = lay.bt_total;
    m.vlen = packed_len(C);
    m.order = lay.cm_mem;
    const std::vector<i32> &order = m.order;
    std::vector<i32> old2new(N), comm_new(N);
    m.D.resize((size_t)N * N); m.w.resize(N); m.T0.resize(N); m.T.assign(N, std::nan(""));
    for (i64 q = 0; q < N; q++) {
        const i64 a = order[q];
        old2new[a] = (i32)q;
        comm_new[q] = hcomm[a];
        m.w[q] = p.w[a]; m.T0[q] = p.T0[a];
        double *dst = m.D.data() + q * N;
        for (i64 r = 0; r < N; r++) dst[r] = p.D[a * N + order[r]];
    }
    for (i64 q = 0; q < N; q++) lay.cm_mem[q] = (i32)q; // the member lists in the new numbering, as plan_layout leaves them
    m.comm.ensure(N);
    HIP_CHECK(hipMemcpyAsync(m.comm.p, comm_new.data(), sizeof(i32) * N, hipMemcpyHostToDevice, st));
    WordPacker pk(c);
    std::vector<i32> cm_pos;
    community_tables(c, lay, N, C, pk, cm_pos);
    pk.flush();
    k_bins_prepare(c, c->sw_cm_off.p, N, C, lay.bt_total);
    HIP_CHECK(hipMemsetAsync(c->sw_bt_part.p, 0xFF, sizeof(double) * lay.bt_total, st)); // (all bits set: a NaN where nothing writes)
    ls_down(c, p.fc, c->sw_bt_fc.p, Nt);
    ls_down(c, p.ns, c->sw_bt_ns.p, Nt);
    ls_down(c, p.base, c->sw_bt_base.p, Nt * Nt);
    // the tally's operands: the caller's, T's indices through old2new
    if (S > 0) {
        std::vector<i32> ax((size_t)4 * S);
        for (i64 k = 0; k < 4 * S; k++) ax[k] = old2new[p.aidx[k]];
        ls_up(c, m.aidx, ax.data(), 4 * S);
        m.afac.ensure((size_t)8 * S + CGE_PARTIAL_BLOCKS); // (the blocks' weight sums behind the factors, as fused_tables keeps them)
        HIP_CHECK(hipMemcpyAsync(m.afac.p, p.afac, sizeof(double) * 8 * S, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(m.afac.p + 8 * S, p.aden, sizeof(double) * CGE_PARTIAL_BLOCKS, hipMemcpyHostToDevice, st));
        ls_up(c, m.dpos, p.dpos, S);
        ls_up(c, m.dneg, p.dneg, S);
        ls_up(c, m.wts, p.wts, S);
        m.apw.ensure((size_t)2 * S);
        HIP_CHECK(hipMemsetAsync(m.apw.p, 0xFF, sizeof(double) * 2 * S, st));
        HIP_CHECK(hipStreamSynchronize(st)); // (ax goes out of scope)
    }
    c->sw_scal.ensure(RES_STRIDE);
    m.epi = fused_entry(c, m.comm.p, S, m.dpos.p, m.dneg.p, m.wts.p);
    if (S > 0) { m.epi.aidx = m.aidx.p; m.epi.afac = m.afac.p; m.epi.aden = m.afac.p + 8 * S; m.epi.apw = m.apw.p; }
    if (shared) { // the tables and the tallies' place leave the context with the member
        m.scal.ensure(2 * CGE_PARTIAL_BLOCKS);
        m.epi.auc_part = m.scal.p;
        HIP_CHECK(hipStreamSynchronize(st));
        m.fc.swap(c->sw_bt_fc); m.ns.swap(c->sw_bt_ns); m.base.swap(c->sw_bt_base); m.part.swap(c->sw_bt_part); m.cm_off.swap(c->sw_cm_off);
        m.epi_dev.ensure(sizeof(cge_fit_fused));
        HIP_CHECK(hipMemcpyAsync(m.epi_dev.p, &m.epi, sizeof(cge_fit_fused), hipMemcpyHostToDevice, st));
    } else
        fused_upload(c, std::vector<cge_fit_fused>(1, m.epi));
    HIP_CHECK(hipMemsetAsync(m.epi.auc_part, 0xFF, sizeof(double) * 2 * CGE_PARTIAL_BLOCKS, st)); // (NaN until the epilogue writes)
    // vect_B with its guard of NaNs behind it, and vect_C (zeros where the caller has none)
    std::vector<double> hv((size_t)(m.vlen + CGE_VECT_B_GUARD), std::nan("")), hc((size_t)m.vlen, 0.0);
    if (p.vC) std::memcpy(hc.data(), p.vC, sizeof(double) * m.vlen);
    ls_up(c, m.vB, hv.data(), (i64)hv.size());
    ls_up(c, m.vC, hc.data(), m.vlen);
    m.fpart.ensure((size_t)2 * CGE_PARTIAL_BLOCKS);
    HIP_CHECK(hipStreamSynchronize(st)); // (the host copies go out of scope)
}

// what a problem's launch left: the iterate in the caller's numbering, the tile partials (before the bins), the tallies, the powers
static void fc_collect(cge_ctx *c, cge_fused_chain_problem &p, FcMember &m, const double *partial) {
    const i64 S = (p.want & 2) ? p.S : 0;
    for (i64 q = 0; q < p.N; q++) p.T[m.order[q]] = m.T[q];
    if (p.order) std::memcpy(p.order, m.order.data(), sizeof(i32) * p.N);
    p.bt_total = m.bt_total;
    ls_down(c, p.partials, partial, m.bt_total);
    ls_down(c, p.part, m.epi.auc_part, 2 * CGE_PARTIAL_BLOCKS);
    if (S > 0) ls_down(c, p.apw, m.apw.p, 2 * S);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

void host_fused_chain_test(cge_ctx *c, cge_fused_chain_problem *probs, int n, double eps, double delta) {
    hipStream_t st = c->stream;
    // ---- the checks that need no layout ------------------------------------------------------------------------------------------
    if (n > CGE_BATCH_MAX) CGE_THROW(CGE_E_ARG, "fused_chain_test: a launch takes at most %d problems", CGE_BATCH_MAX);
    if (!(eps > 0.0) || !(delta >= 0.0)) CGE_THROW(CGE_E_ARG, "fused_chain_test: eps > 0 and delta >= 0");
    if (!c->opt_pow_exp2)
        CGE_THROW(CGE_E_ARG, "fused_chain_test: the fused fit makes its power matrix from the stored logarithm (option pow_exp2)");
    if (c->fit_persistent_broken) CGE_THROW(CGE_E_ARG, "fused_chain_test: this context gave the persistent fit up");
    FlowGeometry geo[CGE_BATCH_MAX];
    const int cus = device_cus();
    int sumG = 0;
    for (int i = 0; i < n; i++) {
        const cge_fused_chain_problem &p = probs[i];
        if (!p.D || !p.w || !p.T0 || !p.comm || !p.T) CGE_THROW(CGE_E_ARG, "fused_chain_test: empty problem");
        if (p.N < 256 || p.C < 2)
            CGE_THROW(CGE_E_ARG, "fused_chain_test: the tiles need 256 vertices and 2 communities (N = %lld, C = %lld)", (long long)p.N, (long long)p.C);
        if ((double)p.N * (double)p.C > 1e9) CGE_THROW(CGE_E_ARG, "fused_chain_test: problem too large");
        if (p.want < 1 || p.want > 3) CGE_THROW(CGE_E_ARG, "fused_chain_test: want = %d (bit 0 vect_B's partials, bit 1 the tallies)", (int)p.want);
        if (p.n_modes < 1 || p.n_modes > 2) CGE_THROW(CGE_E_ARG, "fused_chain_test: n_modes = %d", (int)p.n_modes);
        if (p.vC && !p.js_fused) CGE_THROW(CGE_E_ARG, "fused_chain_test: vC without js_fused");
        if (p.want & 2) {
            if (p.S < 1 || p.S > 65535) CGE_THROW(CGE_E_ARG, "fused_chain_test: S = %lld samples (1 .. 65535)", (long long)p.S);
            if (!p.aidx || !p.afac || !p.aden || !p.dpos || !p.dneg || !p.wts)
                CGE_THROW(CGE_E_ARG, "fused_chain_test: the tallies take aidx, afac, aden, dpos, dneg and wts");
            for (i64 k = 0; k < 4 * p.S; k++)
                if (p.aidx[k] < 0 || p.aidx[k] >= p.N)
                    CGE_THROW(CGE_E_ARG, "fused_chain_test: aidx[%lld] = %d outside 0..%lld", (long long)k, (int)p.aidx[k], (long long)(p.N - 1));
        }
        if (!(flow_geometry(p.N, cus, &geo[i]) && geo[i].fused()))
            CGE_THROW(CGE_E_ARG, "fused_chain_test: the geometry of the fused persistent fit declines N = %lld on %d CUs", (long long)p.N, cus);
        if (geo[i].NW != geo[0].NW)
            CGE_THROW(CGE_E_ARG, "fused_chain_test: a launch takes problems of one NW (problem %d runs %d waves per workgroup, problem 0 runs %d)", i,
                      geo[i].NW, geo[0].NW);
        sumG += geo[i].G;
    }
    if (n > 1 && sumG > cus)
        CGE_THROW(CGE_E_ARG, "fused_chain_test: the problems need %d workgroups in all, the device has %d CUs", sumG, cus);
    if (n > 1 && !k_fit_flow_multi_fits(geo[0].NW, false))
        CGE_THROW(CGE_E_ARG, "fused_chain_test: fit_flow_multi_kernel of %d waves gets no workgroup on a CU", geo[0].NW);
    FcOptions restore(c);
    c->opt_fit_fused = 1; c->opt_exact_relabel = true; c->opt_test_bvec_plain = 0;
    if (c->opt_fit_persistent == 1) c->opt_fit_persistent = 0;
    std::vector<std::unique_ptr<FcMember>> mem;
    if (n == 1) { // ---- fit_flow_kernel<.., true>, as enqueue_alpha launches it, then bins_js_kernel -------------------------------
        cge_fused_chain_problem &p = probs[0];
        mem.emplace_back(new FcMember());
        FcMember &m = *mem.back();
        fc_prepare(c, p, m, false);
        cge_fit_problem fp{};
        fp.D = m.D.data(); fp.w = m.w.data(); fp.T0 = m.T0.data(); fp.T = m.T.data(); fp.N = p.N; fp.alpha = p.alpha;
        ft_undirected(c, fp, 4, eps, delta, &m.epi, reinterpret_cast<const cge_fit_fused *>(c->sw_fused_epi.p), p.want);
        p.iters = fp.iters;
        p.status = fp.status;
        fc_collect(c, p, m, c->sw_bt_part.p);
        if ((p.want & 1) && p.status == 0) k_bins_js(c, c->sw_cm_off.p, p.N, p.C, m.vC.p, m.vB.p, p.n_modes, m.fpart.p);
    } else { // ---- fit_flow_multi_kernel over the members, then the batch's bins / JS launches ------------------------------------------
        DevBuf<int> flags;
        DevBuf<double> flow;
        flags.ensure((size_t)4 * n);
        HIP_CHECK(hipMemsetAsync(flags.p, 0, sizeof(int) * 4 * n, st));
        cge_flow_multi tab{};
        tab.n = n;
        std::vector<cge_fit_problem> fps(n);
        for (int i = 0; i < n; i++) {
            const cge_fused_chain_problem &p = probs[i];
            mem.emplace_back(new FcMember());
            FcMember &m = *mem.back();
            fc_prepare(c, p, m, true);
            cge_fit_problem &fp = fps[i];
            fp = cge_fit_problem{};
            fp.D = m.D.data(); fp.w = m.w.data(); fp.T0 = m.T0.data(); fp.T = m.T.data(); fp.N = p.N; fp.alpha = p.alpha;
            tab.p[i] = ft_member(c, fp, geo[i], m.fit, flags.p + 4 * i, reinterpret_cast<const cge_fit_fused *>(m.epi_dev.p), p.want);
        }
        k_fit_flow_multi(c, tab, geo[0].NW, eps, delta, flow);
        ft_multi_collect(c, fps.data(), n, tab);
        cge_bins_multi bins{};
        cge_js_multi js{};
        int nb = 0, nj = 0;
        i64 maxC = 0;
        for (int i = 0; i < n; i++) {
            cge_fused_chain_problem &p = probs[i];
            FcMember &m = *mem[i];
            p.iters = fps[i].iters;
            p.status = fps[i].status;
            fc_collect(c, p, m, m.part.p);
            if (!((p.want & 1) && p.status == 0)) continue;
            bins.p[nb++] = cge_bins_problem{m.part.p, m.cm_off.p, m.fc.p, m.ns.p, m.base.p, p.C, geo[i].Nt, 0, m.vB.p};
            maxC = std::max(maxC, p.C);
            m.jspart.ensure((size_t)2 * 3 * CGE_PARTIAL_BLOCKS);
            for (int u = 0; u < p.n_modes; u++, nj++)
                js.p[nj] = cge_js_problem{m.vC.p, m.vB.p, m.vlen, p.C, p.n_modes == 1 ? 0 : 1 + u, 0, m.jspart.p + (i64)u * 3 * CGE_PARTIAL_BLOCKS,
                                          m.fpart.p + (i64)u * CGE_PARTIAL_BLOCKS};
        }
        k_bins_js_multi(c, bins, nb, maxC, js, nj);
    }
    for (int i = 0; i < n; i++) {
        cge_fused_chain_problem &p = probs[i];
        FcMember &m = *mem[i];
        std::vector<double> hf((size_t)2 * CGE_PARTIAL_BLOCKS, std::nan(""));
        const bool binned = (p.want & 1) && p.status == 0;
        if (binned) ls_down(c, hf.data(), m.fpart.p, 2 * CGE_PARTIAL_BLOCKS);
        ls_down(c, p.vectB, m.vB.p, m.vlen + CGE_VECT_B_GUARD);
        HIP_CHECK(hipStreamSynchronize(st));
        if (p.vC)
            for (int u = 0; u < p.n_modes; u++) p.js_fused[u] = binned ? vb_fold(hf.data() + (i64)u * CGE_PARTIAL_BLOCKS) : std::nan("");
    }
}

// ---- the testing hook of the local score (include/cge_hip_testing.h: cge_local_score_test) -----------------------------------
// The stages of the local score on the buffers a sweep keeps them in (the first DevSamples of the context): the device sampler,
// k_prep_samples, sampled_pair_dist and the tallies -- k_auc_landmark / k_auc_exact, or the epilogue of the fused fit through
// fused_tables and ft_undirected.  Every check comes before the first launch.
static void ls_range(const char *what, const i32 *v, i64 cnt, i64 lim) {
    for (i64 k = 0; k < cnt; k++)
        if (v[k] < 0 || v[k] >= lim)
            CGE_THROW(CGE_E_ARG, "local_score_test: %s[%lld] = %d outside 0..%lld", what, (long long)k, (int)v[k], (long long)(lim - 1));
}

void host_local_score_test(cge_ctx *c, cge_local_score_io *io) {
    hipStream_t st = c->stream;
    const i64 S = io->S, n = c->n, m = c->m, N = io->N;
    const int directed = io->directed != 0, form = io->form;
    const bool landmark_form = form == 1 || form == 4, exact_form = form == 2 || form == 3;
    // the stages that run
    const bool draw = io->draw_route != 0;
    const bool pairs_in = io->pi_in || io->pj_in || io->ni_in || io->nj_in || io->wts_in;
    const bool draws_in = io->pos_in || io->neg_i_in || io->neg_j_in;
    const bool dist = io->dpos || io->dneg || (landmark_form && !io->dpos_in);
    const bool prep = io->pi || io->pj || io->ni || io->nj || io->wts || ((dist || form != 0) && !pairs_in);
    // ---- the checks --------------------------------------------------------------------------------------------------------------
    if (S < 1 || S >= ((i64)1 << 28)) CGE_THROW(CGE_E_ARG, "local_score_test: S = %lld samples", (long long)S);
    if (c->rows_sharded || c->edges_sharded)
        CGE_THROW(CGE_E_ARG, "local_score_test: not with option shard_rows / shard_ingest (every row and edge on one rank)");
    if ((draw || prep) && (!c->src.p || !c->dst.p || m <= 0 || n < 2 || (!c->unit_weights && !c->w.p)))
        CGE_THROW(CGE_E_ARG, "local_score_test: the graph is not resident (cge_set_graph)");
    if (prep && pairs_in) CGE_THROW(CGE_E_ARG, "local_score_test: the pairs are prepared or supplied, not both");
    if (pairs_in && (!io->pi_in || !io->pj_in || !io->ni_in || !io->nj_in || !io->wts_in))
        CGE_THROW(CGE_E_ARG, "local_score_test: supplied pairs are pi_in, pj_in, ni_in, nj_in and wts_in together");
    if (draws_in && (!io->pos_in || !io->neg_i_in || !io->neg_j_in))
        CGE_THROW(CGE_E_ARG, "local_score_test: supplied draws are pos_in, neg_i_in and neg_j_in together");
    if (prep && !draws_in && !draw) CGE_THROW(CGE_E_ARG, "local_score_test: Prepare takes pos_in, neg_i_in and neg_j_in, or a draw");
    if (io->pos2_in && !prep) CGE_THROW(CGE_E_ARG, "local_score_test: pos2_in goes with Prepare");
    if ((io->dpos_in != nullptr) != (io->dneg_in != nullptr)) CGE_THROW(CGE_E_ARG, "local_score_test: dpos_in and dneg_in go together");
    if (io->dpos_in && form == 0) CGE_THROW(CGE_E_ARG, "local_score_test: dpos_in and dneg_in go with a tally");
    if ((landmark_form || dist) && n < 1) CGE_THROW(CGE_E_ARG, "local_score_test: nothing is resident");
    if (dist && (!c->Xr.p || c->d <= 0 || c->Xr.n < (size_t)(n * c->d)))
        CGE_THROW(CGE_E_ARG, "local_score_test: the embedding is not resident (cge_set_embedding)");
    if (dist && !(io->hi > 0.0)) CGE_THROW(CGE_E_ARG, "local_score_test: hi = %g (the distances are divided by it)", io->hi);
    if (form != 0 && (N < 1 || N > 46340)) CGE_THROW(CGE_E_ARG, "local_score_test: N = %lld", (long long)N);
    if (exact_form && prep && N != n)
        CGE_THROW(CGE_E_ARG, "local_score_test: forms 2 and 3 on prepared pairs take N = n (N = %lld, n = %lld)", (long long)N, (long long)n);
    if (draws_in && prep) {
        ls_range("pos_in", io->pos_in, S, m);
        ls_range("neg_i_in", io->neg_i_in, S, n);
        ls_range("neg_j_in", io->neg_j_in, S, n);
    }
    if (io->pos2_in) ls_range("pos2_in", io->pos2_in, S, m);
    if (pairs_in) {
        const i64 lim = exact_form ? (dist ? std::min(N, n) : N) : n;
        ls_range("pi_in", io->pi_in, S, lim);
        ls_range("pj_in", io->pj_in, S, lim);
        ls_range("ni_in", io->ni_in, S, lim);
        ls_range("nj_in", io->nj_in, S, lim);
    }
    if (landmark_form) {
        if (!io->v2l || !io->vw || !io->lweight) CGE_THROW(CGE_E_ARG, "local_score_test: forms 1 and 4 take v2l, vw and lweight");
        ls_range("v2l", io->v2l, n, N);
        if (io->old2new) {
            ls_range("old2new", io->old2new, N, N);
            std::vector<char> seen(N, 0);
            for (i64 l = 0; l < N; l++) {
                if (seen[io->old2new[l]]) CGE_THROW(CGE_E_ARG, "local_score_test: old2new is not a permutation (%d twice)", (int)io->old2new[l]);
                seen[io->old2new[l]] = 1;
            }
        }
    }
    if (form == 1 && !io->Ta) CGE_THROW(CGE_E_ARG, "local_score_test: form 1 takes Ta");
    if (exact_form && (!io->GD || !io->Ta)) CGE_THROW(CGE_E_ARG, "local_score_test: forms 2 and 3 take GD and Ta");
    if ((form == 3 || form == 4) && directed) CGE_THROW(CGE_E_ARG, "local_score_test: form %d is undirected only", form);
    if (form == 4) {
        if (!io->D || !io->w || !io->T0) CGE_THROW(CGE_E_ARG, "local_score_test: form 4 takes D, w and T0");
        if (!(io->eps > 0.0) || !(io->delta >= 0.0)) CGE_THROW(CGE_E_ARG, "local_score_test: eps > 0 and delta >= 0");
        if (!c->opt_pow_exp2)
            CGE_THROW(CGE_E_ARG, "local_score_test: form 4 makes its power matrix from the stored logarithm (option pow_exp2)");
        if (!flow_fused_applies(N))
            CGE_THROW(CGE_E_ARG, "local_score_test: the geometry of the fused persistent fit declines N = %lld", (long long)N);
    }
    // ---- Draw --------------------------------------------------------------------------------------------------------------------
    while (c->dsets.empty()) c->dsets.emplace_back(new DevSamples());
    DevSamples &ds = *c->dsets[0];
    DevBuf<i32> d_pos, d_pos2, d_ni, d_nj;
    io->rounds = 0;
    if (draw) {
        d_pos.ensure(S); d_ni.ensure(S); d_nj.ensure(S);
        if (io->draw_route == 1)
            k_draw_samples_dev(c, io->seed, io->stream_id, S, directed, d_pos.p, d_ni.p, d_nj.p);
        else {
            k_draw_samples_begin(c, io->seed, io->stream_id, S, directed, d_pos.p, d_ni.p, d_nj.p);
            k_draw_samples_finish(c);
        }
        io->rounds = c->samp_pending.round;
        ls_down(c, io->pos, d_pos.p, S);
        ls_down(c, io->neg_i, d_ni.p, S);
        ls_down(c, io->neg_j, d_nj.p, S);
        ls_down(c, io->attempt, c->samp_attempt.p, S);
    }
    // ---- Prepare -----------------------------------------------------------------------------------------------------------------
    if (prep) {
        if (draws_in) {
            ls_up(c, d_pos, io->pos_in, S);
            ls_up(c, d_ni, io->neg_i_in, S);
            ls_up(c, d_nj, io->neg_j_in, S);
        }
        if (io->pos2_in) ls_up(c, d_pos2, io->pos2_in, S);
        ds.pi.ensure(S); ds.pj.ensure(S); ds.ni.ensure(S); ds.nj.ensure(S); ds.wts.ensure(S);
        k_prep_samples(c, d_pos.p, io->pos2_in ? d_pos2.p : d_pos.p, d_ni.p, d_nj.p, c->src.p, c->dst.p, c->w.p, S, directed, ds.pi.p,
                       ds.pj.p, ds.ni.p, ds.nj.p, ds.wts.p);
        ls_down(c, io->pi, ds.pi.p, S);
        ls_down(c, io->pj, ds.pj.p, S);
        ls_down(c, io->ni, ds.ni.p, S);
        ls_down(c, io->nj, ds.nj.p, S);
        ls_down(c, io->wts, ds.wts.p, S);
    } else if (pairs_in) {
        ls_up(c, ds.pi, io->pi_in, S);
        ls_up(c, ds.pj, io->pj_in, S);
        ls_up(c, ds.ni, io->ni_in, S);
        ls_up(c, ds.nj, io->nj_in, S);
        ls_up(c, ds.wts, io->wts_in, S);
    }
    // ---- Distances ---------------------------------------------------------------------------------------------------------------
    if (dist) {
        ds.dpos.ensure(S); ds.dneg.ensure(S);
        sampled_pair_dist(c, c->Xr.p, c->d, ds.pi.p, ds.pj.p, S, io->hi, ds.dpos.p);
        sampled_pair_dist(c, c->Xr.p, c->d, ds.ni.p, ds.nj.p, S, io->hi, ds.dneg.p);
        ls_down(c, io->dpos, ds.dpos.p, S);
        ls_down(c, io->dneg, ds.dneg.p, S);
    }
    if (io->dpos_in) { // (behind the copies out of the distance stage, when that ran for its outputs)
        ls_up(c, ds.dpos, io->dpos_in, S);
        ls_up(c, ds.dneg, io->dneg_in, S);
    }
    // ---- Tally -------------------------------------------------------------------------------------------------------------------
    DevBuf<double> dTa, dTb, dvw, dlw, dout2;
    DevBuf<i32> dv2l, do2n;
    std::vector<double> hpart(2 * CGE_PARTIAL_BLOCKS, std::nan(""));
    if (landmark_form) {
        ls_up(c, dv2l, io->v2l, n);
        ls_up(c, dvw, io->vw, n);
        ls_up(c, dlw, io->lweight, N);
        if (io->old2new) ls_up(c, do2n, io->old2new, N);
    }
    if (form >= 1 && form <= 3) {
        ls_up(c, dTa, io->Ta, N);
        if (io->Tb) ls_up(c, dTb, io->Tb, N);
        dout2.ensure(2);
    }
    if (form == 1) {
        const double *Ta = dTa.p, *Tb = io->Tb ? dTb.p : dTa.p;
        if (io->old2new) { // T is stored in sweep order: un-permuted, as local_score_tallies does
            c->sw_rl_T.ensure((size_t)2 * N);
            k_permute_rows(c, Ta, do2n.p, N, 1, c->sw_rl_T.p);
            Ta = c->sw_rl_T.p;
            if (io->Tb) {
                k_permute_rows(c, Tb, do2n.p, N, 1, c->sw_rl_T.p + N);
                Tb = c->sw_rl_T.p + N;
            } else
                Tb = Ta;
        }
        k_auc_landmark(c, Ta, Tb, dv2l.p, dvw.p, dlw.p, ds.pi.p, ds.pj.p, ds.ni.p, ds.nj.p, ds.dpos.p, ds.dneg.p, ds.wts.p, S, io->alpha,
                       dout2.p);
    } else if (exact_form) {
        const bool packed = form == 3;
        const i64 Nt = (N + 63) / 64;
        std::vector<double> pk;
        if (packed) { // the upper tiles of GD, zeros outside the matrix, through the address inline every consumer uses
            pk.assign((size_t)(Nt * (Nt + 1) / 2) * CGE_TILE_DOUBLES, 0.0);
            for (i64 i = 0; i < N; i++)
                for (i64 j = i / 64 * 64; j < N; j++) pk[cge_packed_index(i, j, Nt)] = io->GD[i * N + j];
            ls_up(c, c->sw_PK, pk.data(), (i64)pk.size());
        } else
            ls_up(c, c->sw_GD, io->GD, N * N);
        k_auc_exact(c, packed ? c->sw_PK.p : c->sw_GD.p, dTa.p, io->Tb ? dTb.p : dTa.p, N, ds.pi.p, ds.pj.p, ds.ni.p, ds.nj.p, ds.wts.p, S,
                    dout2.p, nullptr, packed);
        HIP_CHECK(hipStreamSynchronize(st)); // (pk goes out of scope)
    }
    if (form >= 1 && form <= 3) {
        ls_down(c, hpart.data(), c->auc_part.p, 2 * CGE_PARTIAL_BLOCKS);
        ls_down(c, io->out2, dout2.p, 2);
    }
    if (form == 4) {
        c->sw_scal.ensure(RES_STRIDE);
        HIP_CHECK(hipMemsetAsync(c->sw_scal.p + RES_AUC, 0xFF, sizeof(double) * 2 * CGE_PARTIAL_BLOCKS, st)); // (NaN until the epilogue writes)
        OrigView orig;
        orig.n = n; orig.v2l = dv2l.p; orig.vw = dvw.p; orig.lweight = dlw.p;
        ScoreGraph G;
        G.N = N;
        std::vector<cge_fit_fused> h_epi;
        fused_tables(c, G, &orig, io->old2new ? do2n.p : nullptr, 1, 0, S, true, h_epi);
        std::vector<double> hT(N);
        cge_fit_problem p{};
        p.D = io->D; p.w = io->w; p.T0 = io->T0; p.T = io->T ? io->T : hT.data(); p.N = N; p.alpha = io->alpha;
        ft_undirected(c, p, 4, io->eps, io->delta, &h_epi[0], reinterpret_cast<const cge_fit_fused *>(c->sw_fused_epi.p));
        io->iters = p.iters;
        io->status = p.status;
        ls_down(c, hpart.data(), c->sw_scal.p + RES_AUC, 2 * CGE_PARTIAL_BLOCKS);
        ls_down(c, io->aidx, ds.aidx.p, 4 * S);
        ls_down(c, io->afac, ds.afac.p, 8 * S);
        ls_down(c, io->aden, ds.afac.p + 8 * S, (i64)CGE_PARTIAL_BLOCKS);
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (form == 3) c->sw_PK.release(); // (held only while packed sweeps run)
    if (form != 0 && io->part) std::memcpy(io->part, hpart.data(), sizeof(double) * hpart.size());
    if (form == 4 && io->out2) { // the block tallies in block order, as the sweep's host adds them
        double num = 0.0, den = 0.0;
        for (int b = 0; b < CGE_PARTIAL_BLOCKS; b++) { num += hpart[2 * b]; den += hpart[2 * b + 1]; }
        io->out2[0] = num;
        io->out2[1] = den;
    }
}

// ---- the testing hook of the sweep's set-up (include/cge_hip_testing.h: cge_sweep_setup_test) ------------------------------------
// What host_wgcl_sweep does before its first alpha, on a caller's score graph and stage by stage: edge_degrees, plan_layout,
// prepare_distances, k_pow_prepare, k_pow_matrix -- the sweep's own functions, on the buffers a host-array sweep keeps them in
// (s_emb .. s_comm, s_degin / s_degout / s_star, sw_*, fp_T).  No fit runs.  Everything that can refuse does so before the first
// launch, but the layout's own verdict on the tiles.
void host_sweep_setup_test(cge_ctx *c, cge_sweep_setup_io *io) {
    hipStream_t st = c->stream;
    const i64 N = io->N, d = io->d, C = io->C, m = io->m;
    const int directed = io->directed != 0, form = io->log_form;
    const bool landmarks = io->landmarks != 0, edges = io->src || io->dst;
    // the stages that run
    const bool want_log = io->Lh || io->Ll, want_gd = io->GD != nullptr;
    const bool want_prep = io->lo_hi || io->D || io->cm_off || io->cm_mem || io->cm_pos || io->T1 || io->T2 || io->TT || want_log || want_gd;
    io->Tld = io->log_count = 0;
    io->relabel = io->log_form_ran = 0;
    // ---- the checks --------------------------------------------------------------------------------------------------------------
    if (N < 1 || d < 1 || C < 1 || N > 46340) CGE_THROW(CGE_E_ARG, "sweep_setup_test: N = %lld, d = %lld, C = %lld", (long long)N, (long long)d, (long long)C);
    if (!io->emb || !io->dist || !io->comm) CGE_THROW(CGE_E_ARG, "sweep_setup_test: emb, dist and comm are the score graph");
    if (c->rows_sharded || c->edges_sharded || c->opt_shard_rows || c->opt_shard_ingest)
        CGE_THROW(CGE_E_ARG, "sweep_setup_test: not with option shard_rows / shard_ingest (every row and edge on one rank)");
    if (form < 0 || form > 3) CGE_THROW(CGE_E_ARG, "sweep_setup_test: log_form = %d (0 .. 3)", form);
    if (form != 0 && !c->opt_pow_exp2) CGE_THROW(CGE_E_ARG, "sweep_setup_test: a stored logarithm needs option pow_exp2");
    if (form == 3 && N < 256) CGE_THROW(CGE_E_ARG, "sweep_setup_test: the tile-blocked logarithm belongs to the fused fit, from 256 vertices on (N = %lld)", (long long)N);
    if (want_log && (!io->Lh || !io->Ll)) CGE_THROW(CGE_E_ARG, "sweep_setup_test: Lh and Ll go together");
    std::vector<i32> hcomm(N);
    for (i64 i = 0; i < N; i++) {
        if (io->comm[i] < 1 || io->comm[i] > C) CGE_THROW(CGE_E_ARG, "sweep_setup_test: community id out of range");
        hcomm[i] = (i32)(io->comm[i] - 1);
    }
    if (edges && (!io->src || !io->dst || m < 1)) CGE_THROW(CGE_E_ARG, "sweep_setup_test: an edge list is src, dst and m >= 1");
    if (directed && !edges) CGE_THROW(CGE_E_ARG, "sweep_setup_test: a directed sweep starts from the degrees of its edge list");
    if ((io->deg_out || io->deg_in || io->star) && !edges) CGE_THROW(CGE_E_ARG, "sweep_setup_test: the degrees need the edge list");
    for (i64 e = 0; edges && e < m; e++)
        if (io->src[e] < 0 || io->src[e] >= N || io->dst[e] < 0 || io->dst[e] >= N)
            CGE_THROW(CGE_E_ARG, "sweep_setup_test: edge %lld (%d, %d) outside 0..%lld", (long long)e, (int)io->src[e], (int)io->dst[e], (long long)(N - 1));
    const i64 Nt = (N + 63) / 64, blocked_len = Nt * (Nt + 1) / 2 * 4096;
    if (want_log && io->log_cap < (form == 3 ? blocked_len : form == 0 ? std::max(blocked_len, N * N) : N * N))
        CGE_THROW(CGE_E_ARG, "sweep_setup_test: Lh / Ll hold %lld elements, the form may write more", (long long)io->log_cap);
    // ---- the score graph on the device, as a host-array sweep holds it --------------------------------------------------------
    c->s_emb.ensure((size_t)N * d); c->s_dist.ensure(N); c->s_comm.ensure(N);
    HIP_CHECK(hipMemcpyAsync(c->s_emb.p, io->emb, sizeof(double) * N * d, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->s_dist.p, io->dist, sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->s_comm.p, hcomm.data(), sizeof(i32) * N, hipMemcpyHostToDevice, st));
    ScoreGraph G;
    G.N = N; G.d = d; G.C = C;
    G.emb = c->s_emb.p; G.dist = c->s_dist.p; G.comm = c->s_comm.p;
    if (io->vw) {
        c->s_vw.ensure(N);
        HIP_CHECK(hipMemcpyAsync(c->s_vw.p, io->vw, sizeof(double) * N, hipMemcpyHostToDevice, st));
        G.vw = c->s_vw.p;
    }
    // ---- the degrees (score_host.cpp: edge_degrees) ----------------------------------------------------------------------------
    DevBuf<i32> e_src, e_dst;
    DevBuf<double> e_w;
    if (edges) {
        e_src.ensure(m); e_dst.ensure(m);
        HIP_CHECK(hipMemcpyAsync(e_src.p, io->src, sizeof(i32) * m, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(e_dst.p, io->dst, sizeof(i32) * m, hipMemcpyHostToDevice, st));
        if (io->w) {
            e_w.ensure(m);
            HIP_CHECK(hipMemcpyAsync(e_w.p, io->w, sizeof(double) * m, hipMemcpyHostToDevice, st));
        }
        edge_degrees(c, e_src.p, e_dst.p, io->w ? e_w.p : nullptr, m, N, c->s_star);
        G.deg_in = c->s_degin.p;
        G.deg_out = c->s_degout.p;
        if (io->deg_out) HIP_CHECK(hipMemcpyAsync(io->deg_out, c->s_degout.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        if (io->deg_in) HIP_CHECK(hipMemcpyAsync(io->deg_in, c->s_degin.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        if (io->star) HIP_CHECK(hipMemcpyAsync(io->star, c->s_star.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    // ---- the layout ----------------------------------------------------------------------------------------------------------------
    c->sw_T1.ensure(N); c->sw_T2.ensure(N);
    c->sw_lohi.ensure(2);
    SweepLayout lay;
    const OrigView orig{}; // (landmark mode: what the layout asks of it is that it is there)
    plan_layout(c, G, landmarks ? &orig : nullptr, directed, lay, false, io->force_relabel != 0);
    if (form == 3 && !c->bvec_blocks)
        CGE_THROW(CGE_E_ARG, "sweep_setup_test: the tiles decline this layout (more than 64 community ids in a 64-vertex block, or no tile form for this sweep)");
    io->relabel = lay.relabel;
    if (lay.relabel) {
        if (io->order) HIP_CHECK(hipMemcpyAsync(io->order, c->sw_rl_order.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
        if (io->old2new) HIP_CHECK(hipMemcpyAsync(io->old2new, lay.old2new.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
    }
    if (io->emb_rl) HIP_CHECK(hipMemcpyAsync(io->emb_rl, G.emb, sizeof(double) * N * d, hipMemcpyDeviceToHost, st));
    if (io->comm_rl) HIP_CHECK(hipMemcpyAsync(io->comm_rl, G.comm, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
    if (io->vec_rl) {
        const double *vec[4] = {G.dist, G.vw, G.deg_in, G.deg_out};
        for (int q = 0; q < 4; q++)
            if (vec[q]) HIP_CHECK(hipMemcpyAsync(io->vec_rl + q * N, vec[q], sizeof(double) * N, hipMemcpyDeviceToHost, st));
    }
    // ---- D, its extrema and normalisation, the community tables, the start vectors ------------------------------------------
    if (io->D_raw || want_prep) { c->sw_D.ensure((size_t)N * N); c->sw_GD.ensure((size_t)N * N); }
    if (io->D_raw) {
        k_dist_matrix(c, G.emb, G.dist, N, d, c->sw_D.p);
        HIP_CHECK(hipMemcpyAsync(io->D_raw, c->sw_D.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (!want_prep) return;
    io->Tld = prepare_distances(c, G, lay, directed, false);
    if (io->lo_hi) HIP_CHECK(hipMemcpyAsync(io->lo_hi, c->sw_lohi.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    if (io->D) HIP_CHECK(hipMemcpyAsync(io->D, c->sw_D.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
    if (io->cm_off) HIP_CHECK(hipMemcpyAsync(io->cm_off, c->sw_cm_off.p, sizeof(i32) * (C + 1), hipMemcpyDeviceToHost, st));
    if (io->cm_mem) HIP_CHECK(hipMemcpyAsync(io->cm_mem, c->sw_cm_mem.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
    if (io->cm_pos) HIP_CHECK(hipMemcpyAsync(io->cm_pos, c->sw_cm_pos.p, sizeof(i32) * N, hipMemcpyDeviceToHost, st));
    if (io->T1) HIP_CHECK(hipMemcpyAsync(io->T1, c->sw_T1.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (io->T2) HIP_CHECK(hipMemcpyAsync(io->T2, c->sw_T2.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (io->TT) HIP_CHECK(hipMemcpyAsync(io->TT, c->fp_T.p, sizeof(double) * 3 * io->Tld, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (!want_log && !want_gd) return;
    // ---- the logarithm, and the power of one alpha from it ------------------------------------------------------------------
    const bool upper = form == 0 ? landmarks && !directed : form >= 2, blocked = form == 0 ? lay.fuse : form == 3;
    const i64 len = blocked ? blocked_len : N * N;
    if (c->opt_pow_exp2) { // (all bits set: a NaN in both; k_pow_prepare's own ensure finds them large enough)
        c->sw_Lh.ensure((size_t)len); c->sw_Ll.ensure((size_t)len);
        HIP_CHECK(hipMemsetAsync(c->sw_Lh.p, 0xFF, sizeof(double) * len, st));
        HIP_CHECK(hipMemsetAsync(c->sw_Ll.p, 0xFF, sizeof(float) * len, st));
    }
    k_pow_prepare(c, c->sw_D.p, N, upper, blocked);
    io->log_form_ran = c->pow_logs_blocked_N == N ? 3 : c->pow_logs_N != N ? 0 : c->pow_logs_upper ? 2 : 1;
    io->log_count = io->log_form_ran == 0 ? 0 : len;
    if (want_log && io->log_form_ran != 0) {
        HIP_CHECK(hipMemcpyAsync(io->Lh, c->sw_Lh.p, sizeof(double) * len, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(io->Ll, c->sw_Ll.p, sizeof(float) * len, hipMemcpyDeviceToHost, st));
    }
    if (want_gd && io->log_form_ran != 3) {
        HIP_CHECK(hipMemsetAsync(c->sw_GD.p, 0xFF, sizeof(double) * N * N, st)); // (as ft_matrices does)
        k_pow_matrix(c, c->sw_D.p, N, io->alpha, c->sw_GD.p, upper);
        HIP_CHECK(hipMemcpyAsync(io->GD, c->sw_GD.p, sizeof(double) * N * N, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

// ---- the testing hook of the packed form (include/cge_hip_testing.h: cge_packed_gd_test) -------------------------------
// The extrema pass and the generator through the sweep's own launch wrappers on a caller's embedding; the tiles are unpacked on
// the host through cge_packed_index: GD[i][j] for j >= i, and both halves of the diagonal tiles.
void host_packed_gd_test(cge_ctx *c, const double *emb, const double *diag, i64 N, i64 d, double alpha, int pow_method, double *lo_hi,
                         double *GD) {
    hipStream_t st = c->stream;
    const i64 Nt = (N + 63) / 64, NT = Nt * (Nt + 1) / 2;
    DevBuf<double> demb, ddiag, dlohi, PK;
    demb.ensure((size_t)N * d); ddiag.ensure(N); dlohi.ensure(2); PK.ensure((size_t)NT * CGE_TILE_DOUBLES);
    HIP_CHECK(hipMemcpyAsync(demb.p, emb, sizeof(double) * N * d, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(ddiag.p, diag, sizeof(double) * N, hipMemcpyHostToDevice, st));
    k_packed_extrema(c, demb.p, ddiag.p, N, d, dlohi.p);
    k_packed_gd(c, demb.p, ddiag.p, N, d, dlohi.p, alpha, pow_method, PK.p);
    std::vector<double> h((size_t)NT * CGE_TILE_DOUBLES);
    HIP_CHECK(hipMemcpyAsync(h.data(), PK.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(lo_hi, dlohi.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (i64 i = 0; i < N; i++)
        for (i64 j = i / 64 * 64; j < N; j++) GD[i * N + j] = h[cge_packed_index(i, j, Nt)];
    for (i64 I = 0; I < Nt; I++) // outside the matrix: zeros, which the fit adds unmasked
        for (i64 J = I; J < Nt; J++)
            for (i64 r = 0; r < 64; r++)
                for (i64 q = 0; q < 64; q++)
                    if ((64 * I + r >= N || 64 * J + q >= N) && h[cge_packed_index(64 * I + r, 64 * J + q, Nt)] != 0.0)
                        CGE_THROW(CGE_E_ASSERT, "packed_gd_test: a non-zero outside the matrix (tile %lld, %lld)", (long long)I, (long long)J);
}

// ---- small helpers ---------------------------------------------------------------------------------

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
