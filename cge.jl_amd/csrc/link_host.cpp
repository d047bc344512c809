// link_host.cpp -- the host side of cge_link_* (include/cge_hip.h): the link model in the context, fitted by a score's own sweep
// or supplied by the caller, its three queries, its draws and its exact AUC (kernels_link.hip).
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

static void link_need_inputs(cge_ctx *c, const char *who) {
    if (!c->Xr.p || c->d <= 0 || !c->src.p || c->n <= 0 || c->m <= 0)
        CGE_THROW(CGE_E_ARG, "%s: embedding and graph must be resident (cge_set_embedding / cge_set_graph)", who);
    if (c->has_coll || c->rccl_comm || c->edges_sharded || c->rows_sharded || c->opt_shard_ingest || c->opt_shard_rows)
        CGE_THROW(CGE_E_ARG, "%s: not under collectives or sharding", who);
}
static void link_need_model(cge_ctx *c, const char *who) {
    if (!c->link.valid) CGE_THROW(CGE_E_ARG, "%s: no link model (cge_link_fit / cge_link_set_model)", who);
}
// 1-based int64 ids -> 0-based int32, checked before anything is enqueued
static void link_ids(const char *who, const char *what, const int64_t *ids, i64 cnt, i64 n, std::vector<i32> &out, size_t at) {
    for (i64 q = 0; q < cnt; q++) {
        if (ids[q] < 1 || ids[q] > n)
            CGE_THROW(CGE_E_ARG, "%s: %s %lld is vertex %lld, outside 1..%lld", who, what, (long long)(q + 1), (long long)ids[q], (long long)n);
        out[at + (size_t)q] = (i32)(ids[q] - 1);
    }
}
// the model's derived table: the largest f_in of every 128 candidates (the top-k filter's bound)
static void link_finish(cge_ctx *c) {
    LinkModel &m = c->link;
    const i64 nt = c->ldn / 128;
    m.ftile.ensure((size_t)nt);
    k_link_tile_max(c, m.f.p + m.n, m.n, nt, m.ftile.p);
    m.keys_ready = false;
    m.excl_ready = false;
    m.fib_ready = false;
    m.valid = true;
}

// ---- cge_link_fit ------------------------------------------------------------------------------------------------------------------
void link_capture(cge_ctx *c, const double *Ta, const double *Tb, i64 N, const i32 *old2new, double alpha) {
    LinkModel &m = c->link;
    m.cap_T.ensure((size_t)2 * N);
    if (old2new) { // dst[v] = src[old2new[v]]: as local_score_tallies un-permutes a relabelled sweep's T
        k_permute_rows(c, Ta, old2new, N, 1, m.cap_T.p);
        k_permute_rows(c, Tb, old2new, N, 1, m.cap_T.p + N);
    } else {
        HIP_CHECK(hipMemcpyAsync(m.cap_T.p, Ta, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
        HIP_CHECK(hipMemcpyAsync(m.cap_T.p + N, Tb, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
    }
    m.cap_have = true;
    m.cap_alpha = alpha;
    m.cap_N = N;
}

void host_link_fit(cge_ctx *c, const cge_score_args *a, int which, double out[7], int *out_len, cge_trace *trace) {
    if (which != CGE_LINK_BEST_LOCAL && which != CGE_LINK_BEST_GLOBAL)
        CGE_THROW(CGE_E_ARG, "link_fit: which = %d is neither CGE_LINK_BEST_LOCAL nor CGE_LINK_BEST_GLOBAL", which);
    if (which == CGE_LINK_BEST_LOCAL && a->auc_samples < 1)
        CGE_THROW(CGE_E_ARG, "link_fit: the best local score needs auc_samples >= 1 (%lld given)", (long long)a->auc_samples);
    link_need_inputs(c, "link_fit");
    LinkModel &m = c->link;
    link_drop(c);
    m.cap_have = false;
    m.cap_which = which;
    struct Disarm { // whatever happens, the next plain score captures nothing
        LinkModel &m;
        ~Disarm() { m.cap_which = 0; }
    } disarm{m};
    host_score(c, a, out, out_len, trace, nullptr, false);
    m.cap_which = 0;
    if (*out_len != 7 || !m.cap_have) return; // a directed star graph's early return, or no best of the wanted kind: no model
    const bool landmarks = a->land != -1;
    const i64 n = c->n, N = m.cap_N;
    m.directed = a->directed ? 1 : 0;
    m.alpha = m.cap_alpha;
    m.hi = m.cap_hi;
    m.pow_form = m.cap_pow;
    m.n = n;
    m.NT = N;
    m.T.ensure((size_t)2 * N);
    HIP_CHECK(hipMemcpyAsync(m.T.p, m.cap_T.p, sizeof(double) * 2 * N, hipMemcpyDeviceToDevice, c->stream));
    m.f.ensure((size_t)2 * n);
    if (landmarks) k_link_expand(c, m.T.p, m.T.p + N, c->v2l.p, c->vw.p, c->lweight.p, n, m.f.p, m.f.p + n);
    else k_link_expand(c, m.T.p, m.T.p + N, nullptr, nullptr, nullptr, n, m.f.p, m.f.p + n);
    link_finish(c);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// ---- cge_link_set_model / cge_link_model_fetch -------------------------------------------------------------------------------------
void host_link_set_model(cge_ctx *c, int directed, double alpha, double hi, const double *f_out, const double *f_in, i64 n) {
    link_need_inputs(c, "link_set_model");
    if (n != c->n) CGE_THROW(CGE_E_ARG, "link_set_model: n = %lld, the resident inputs have %lld vertices", (long long)n, (long long)c->n);
    if (!std::isfinite(alpha) || alpha <= 0.0) CGE_THROW(CGE_E_ARG, "link_set_model: alpha = %g is not a positive finite number", alpha);
    if (!std::isfinite(hi) || hi <= 0.0) CGE_THROW(CGE_E_ARG, "link_set_model: hi = %g is not a positive finite number", hi);
    if (!directed && f_in && f_in != f_out)
        CGE_THROW(CGE_E_ARG, "link_set_model: an undirected model has one factor per vertex (f_in must be NULL)");
    for (int s = 0; s < 2; s++) {
        const double *f = s ? f_in : f_out;
        if (!f) continue;
        for (i64 v = 0; v < n; v++)
            if (!std::isfinite(f[v]) || f[v] < 0.0)
                CGE_THROW(CGE_E_ARG, "link_set_model: %s[%lld] = %g is negative or not finite", s ? "f_in" : "f_out", (long long)(v + 1), f[v]);
    }
    LinkModel &m = c->link;
    link_drop(c);
    m.directed = directed ? 1 : 0;
    m.alpha = alpha;
    m.hi = hi;
    m.pow_form = 0;
    m.n = n;
    m.NT = 0;
    m.f.ensure((size_t)2 * n);
    HIP_CHECK(hipMemcpyAsync(m.f.p, f_out, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(m.f.p + n, f_in ? f_in : f_out, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    link_finish(c);
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (the caller's arrays are borrowed for the call)
}

void host_link_model_fetch(cge_ctx *c, int *directed, double *alpha, double *hi, double *f_out, double *f_in, double *T_out,
                           double *T_in, int64_t *N) {
    link_need_model(c, "link_model_fetch");
    const LinkModel &m = c->link;
    if (directed) *directed = m.directed;
    if (alpha) *alpha = m.alpha;
    if (hi) *hi = m.hi;
    if (N) *N = m.NT;
    hipStream_t st = c->stream;
    if (f_out) HIP_CHECK(hipMemcpyAsync(f_out, m.f.p, sizeof(double) * m.n, hipMemcpyDeviceToHost, st));
    if (f_in) HIP_CHECK(hipMemcpyAsync(f_in, m.f.p + m.n, sizeof(double) * m.n, hipMemcpyDeviceToHost, st));
    if (T_out && m.NT > 0) HIP_CHECK(hipMemcpyAsync(T_out, m.T.p, sizeof(double) * m.NT, hipMemcpyDeviceToHost, st));
    if (T_in && m.NT > 0) HIP_CHECK(hipMemcpyAsync(T_in, m.T.p + m.NT, sizeof(double) * m.NT, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// ---- cge_link_prob -----------------------------------------------------------------------------------------------------------------
void host_link_prob(cge_ctx *c, const int64_t *i, const int64_t *j, i64 P, double *out) {
    link_need_model(c, "link_prob");
    if (P < 1) CGE_THROW(CGE_E_ARG, "link_prob: P = %lld pairs", (long long)P);
    LinkModel &m = c->link;
    std::vector<i32> h((size_t)2 * P);
    link_ids("link_prob", "i of pair", i, P, m.n, h, 0);
    link_ids("link_prob", "j of pair", j, P, m.n, h, (size_t)P);
    m.ids.ensure((size_t)2 * P);
    m.vals.ensure((size_t)P);
    hipStream_t st = c->stream;
    HIP_CHECK(hipMemcpyAsync(m.ids.p, h.data(), sizeof(i32) * 2 * P, hipMemcpyHostToDevice, st));
    k_link_prob(c, m.ids.p, m.ids.p + P, P, m.vals.p);
    HIP_CHECK(hipMemcpyAsync(out, m.vals.p, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    flush_timers(c);
}

// ---- cge_link_topk -----------------------------------------------------------------------------------------------------------------
// The queries go in chunks of 16384 (128 row tiles): the lists' scratch and the gathered query operand stay bounded, and a chunk
// of that size already fills the device.
void host_link_topk(cge_ctx *c, const int64_t *queries, i64 Q, i64 k, int exclude_edges, int64_t *out_j, double *out_p,
                    int64_t *out_cnt) {
    link_need_model(c, "link_topk");
    if (k < 1 || k > 64) CGE_THROW(CGE_E_ARG, "link_topk: k = %lld is outside 1..64", (long long)k);
    if (Q < 1) CGE_THROW(CGE_E_ARG, "link_topk: Q = %lld queries", (long long)Q);
    LinkModel &m = c->link;
    std::vector<i32> h((size_t)Q);
    link_ids("link_topk", "query", queries, Q, m.n, h, 0);
    hipStream_t st = c->stream;
    host_ensure_centred(c);
    if (exclude_edges) k_link_keys(c);
    const i64 chunk = 16384;
    const i64 cq = std::min(Q, chunk);
    m.ids.ensure((size_t)Q);
    m.oj.ensure((size_t)cq * k);
    m.vals.ensure((size_t)cq * k);
    m.ocnt.ensure((size_t)cq);
    m.surv.ensure(1);
    HIP_CHECK(hipMemcpyAsync(m.ids.p, h.data(), sizeof(i32) * Q, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(m.surv.p, 0, sizeof(unsigned long long), st));
    for (i64 q0 = 0; q0 < Q; q0 += chunk) {
        const i64 nq = std::min(chunk, Q - q0);
        k_link_topk(c, m.ids.p + q0, nq, (int)k, exclude_edges != 0, m.oj.p, m.vals.p, m.ocnt.p);
        HIP_CHECK(hipMemcpyAsync(out_j + q0 * k, m.oj.p, sizeof(i64) * nq * k, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out_p + q0 * k, m.vals.p, sizeof(double) * nq * k, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out_cnt + q0, m.ocnt.p, sizeof(i64) * nq, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st)); // (the next chunk reuses the device outputs)
    }
    unsigned long long surv = 0;
    HIP_CHECK(hipMemcpy(&surv, m.surv.p, sizeof(surv), hipMemcpyDeviceToHost));
    m.stat_survivors = (i64)surv;
    m.stat_queries = Q;
    flush_timers(c);
}

// ---- cge_link_rank -----------------------------------------------------------------------------------------------------------------
// The pairs' own probabilities come from k_link_prob (the same kernel, hence the same bits) and are fetched: the grouping by query
// vertex and the sort of a query's pairs by p descending are done HERE, on the host (P doubles, one synchronisation).  The distinct
// queries go through the counting kernel in chunks of 16384, as top-k's do; one finalisation over all of them follows.
void host_link_rank(cge_ctx *c, const int64_t *i, const int64_t *j, i64 P, int exclude_edges, int64_t *out_greater,
                    int64_t *out_ties, int64_t *out_cand, double *out_p) {
    link_need_model(c, "link_rank");
    link_need_inputs(c, "link_rank");
    if (P < 1) CGE_THROW(CGE_E_ARG, "link_rank: P = %lld pairs", (long long)P);
    LinkModel &m = c->link;
    std::vector<i32> h((size_t)2 * P);
    link_ids("link_rank", "i of pair", i, P, m.n, h, 0);
    link_ids("link_rank", "j of pair", j, P, m.n, h, (size_t)P);
    for (i64 q = 0; q < P; q++)
        if (i[q] == j[q])
            CGE_THROW(CGE_E_ARG, "link_rank: pair %lld is (%lld, %lld): a vertex is not its own candidate", (long long)(q + 1),
                      (long long)i[q], (long long)j[q]);
    hipStream_t st = c->stream;
    const bool exclude = exclude_edges != 0;
    // the pairs' own values
    m.ids.ensure((size_t)2 * P);
    m.vals.ensure((size_t)P);
    HIP_CHECK(hipMemcpyAsync(m.ids.p, h.data(), sizeof(i32) * 2 * P, hipMemcpyHostToDevice, st));
    k_link_prob(c, m.ids.p, m.ids.p + P, P, m.vals.p);
    std::vector<double> p((size_t)P);
    HIP_CHECK(hipMemcpyAsync(p.data(), m.vals.p, sizeof(double) * P, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // grouped by query, a query's pairs by p descending (a NaN -- a non-finite embedding -- last; equal values in the caller's order)
    std::vector<i64> perm((size_t)P);
    std::iota(perm.begin(), perm.end(), (i64)0);
    const i32 *hi_ = h.data();
    std::sort(perm.begin(), perm.end(), [&](i64 a, i64 b) {
        if (hi_[a] != hi_[b]) return hi_[a] < hi_[b];
        const double pa = p[(size_t)a], pb = p[(size_t)b];
        const bool na = std::isnan(pa), nb = std::isnan(pb);
        if (na || nb) return na != nb ? nb : a < b;
        if (pa != pb) return pa > pb;
        return a < b;
    });
    std::vector<i32> uq, gj((size_t)P);
    std::vector<i64> off;
    std::vector<double> t((size_t)P);
    for (i64 s = 0; s < P; s++) {
        const i64 at = perm[(size_t)s];
        if (s == 0 || hi_[at] != uq.back()) {
            uq.push_back(hi_[at]);
            off.push_back(s);
        }
        gj[(size_t)s] = h[(size_t)(P + at)];
        t[(size_t)s] = p[(size_t)at];
    }
    off.push_back(P);
    const i64 Qu = (i64)uq.size();
    m.ruq.ensure((size_t)Qu);
    m.roff.ensure((size_t)Qu + 1);
    m.rgj.ensure((size_t)P);
    m.rperm.ensure((size_t)P);
    m.rt.ensure((size_t)P);
    m.rhist.ensure((size_t)2 * P);
    m.rout.ensure((size_t)3 * P);
    m.surv.ensure(1);
    HIP_CHECK(hipMemcpyAsync(m.ruq.p, uq.data(), sizeof(i32) * Qu, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.roff.p, off.data(), sizeof(i64) * (Qu + 1), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.rgj.p, gj.data(), sizeof(i32) * P, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.rperm.p, perm.data(), sizeof(i64) * P, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.rt.p, t.data(), sizeof(double) * P, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(m.rhist.p, 0, sizeof(unsigned long long) * 2 * P, st));
    HIP_CHECK(hipMemsetAsync(m.surv.p, 0, sizeof(unsigned long long), st));
    host_ensure_centred(c);
    if (exclude) k_link_excl(c); // (and the sorted keys it is derived from)
    unsigned long long *G = m.rhist.p, *E = m.rhist.p + P;
    const i64 chunk = 16384;
    for (i64 q0 = 0; q0 < Qu; q0 += chunk) k_link_rank(c, m.ruq.p + q0, m.roff.p + q0, std::min(chunk, Qu - q0), m.rt.p, G, E, exclude);
    k_link_rank_final(c, m.ruq.p, m.roff.p, Qu, m.rt.p, m.rgj.p, m.rperm.p, G, E, exclude, m.rout.p, m.rout.p + P, m.rout.p + 2 * P);
    HIP_CHECK(hipMemcpyAsync(out_greater, m.rout.p, sizeof(i64) * P, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(out_ties, m.rout.p + P, sizeof(i64) * P, hipMemcpyDeviceToHost, st));
    if (out_cand) HIP_CHECK(hipMemcpyAsync(out_cand, m.rout.p + 2 * P, sizeof(i64) * P, hipMemcpyDeviceToHost, st));
    unsigned long long surv = 0;
    HIP_CHECK(hipMemcpyAsync(&surv, m.surv.p, sizeof(surv), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st)); // (the host tables above are borrowed by the copies until here)
    if (out_p) std::copy(p.begin(), p.end(), out_p);
    m.stat_rank_survivors = (i64)surv;
    m.stat_rank_queries = Qu;
    flush_timers(c);
}

// ---- cge_link_sample ---------------------------------------------------------------------------------------------------------------
// One launch appends the keys of the sampled pairs and counts them; the count is fetched (one synchronisation) and decides: beyond
// cap nothing more is done.  Otherwise the keys are sorted, taken apart, and -- when wanted -- given to k_link_prob (the same
// kernel as cge_link_prob, hence the same bits).
void host_link_sample(cge_ctx *c, i64 seed, i64 stream_id, i64 cap, int64_t *out_i, int64_t *out_j, double *out_p, int64_t *n_edges,
                      const double *U, int directed_layout) {
    const char *who = U ? "link_sample_test" : "link_sample";
    link_need_model(c, who);
    link_need_inputs(c, who);
    if (cap < 0) CGE_THROW(CGE_E_ARG, "%s: cap = %lld", who, (long long)cap);
    if (cap > 0 && (!out_i || !out_j)) CGE_THROW(CGE_E_ARG, "%s: cap = %lld without out_i / out_j", who, (long long)cap);
    LinkModel &m = c->link;
    if (U && m.n > 1024) CGE_THROW(CGE_E_ARG, "%s: n = %lld is beyond the hook's 1024 vertices", who, (long long)m.n);
    hipStream_t st = c->stream;
    host_ensure_centred(c);
    m.scnt.ensure(2);
    m.skeys_in.ensure((size_t)std::max<i64>(cap, 1));
    HIP_CHECK(hipMemsetAsync(m.scnt.p, 0, 2 * sizeof(unsigned long long), st));
    DevBuf<double> dU;
    if (U) {
        dU.ensure((size_t)m.n * m.n);
        HIP_CHECK(hipMemcpyAsync(dU.p, U, sizeof(double) * m.n * m.n, hipMemcpyHostToDevice, st));
    }
    const i64 tiles = k_link_sample(c, seed, stream_id, m.skeys_in.p, cap, m.scnt.p, U ? dU.p : nullptr, directed_layout);
    unsigned long long cnt[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(cnt, m.scnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const i64 ne = (i64)cnt[0];
    *n_edges = ne;
    m.stat_sample_edges = ne;
    m.stat_sample_survivors = (i64)cnt[1];
    m.stat_sample_tiles = tiles;
    if (cap > 0 && ne > cap) {
        flush_timers(c);
        CGE_THROW(CGE_E_ARG, "%s: the sample has n_edges = %lld, cap = %lld is too small", who, (long long)ne, (long long)cap);
    }
    if (cap > 0 && ne > 0) {
        m.skeys.ensure((size_t)ne);
        m.ids.ensure((size_t)2 * ne);
        m.sout.ensure((size_t)2 * ne);
        k_link_sample_finish(c, m.skeys_in.p, m.skeys.p, ne, m.ids.p, m.ids.p + ne, m.sout.p, m.sout.p + ne);
        HIP_CHECK(hipMemcpyAsync(out_i, m.sout.p, sizeof(i64) * ne, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(out_j, m.sout.p + ne, sizeof(i64) * ne, hipMemcpyDeviceToHost, st));
        if (out_p) {
            m.vals.ensure((size_t)ne);
            k_link_prob(c, m.ids.p, m.ids.p + ne, ne, m.vals.p);
            HIP_CHECK(hipMemcpyAsync(out_p, m.vals.p, sizeof(double) * ne, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
    }
    flush_timers(c);
}

// ---- cge_link_auc ------------------------------------------------------------------------------------------------------------------
// The positives' values are k_link_prob's of the resident rows (the same kernel as cge_link_prob, hence the same bits), sorted on
// the device; one launch places the negatives of this part's tiles among them, a prefix sum and a scatter give the counts in the
// edge list's order.  One synchronisation; the three sums are taken here, in the list's order, in long double.
void host_link_auc(cge_ctx *c, int part, int nparts, int64_t *out_less, int64_t *out_ties, double *out_p, int64_t *n_neg,
                   double summary[3]) {
    link_need_model(c, "link_auc");
    link_need_inputs(c, "link_auc");
    if (nparts < 1 || part < 0 || part >= nparts)
        CGE_THROW(CGE_E_ARG, "link_auc: part = %d of nparts = %d (0 <= part < nparts, nparts >= 1)", part, nparts);
    LinkModel &m = c->link;
    const i64 ne = c->m, n = m.n;
    hipStream_t st = c->stream;
    // the call's scratch: values, thresholds, permutation, G and E, the two result arrays -- 56 bytes per edge, grow-only
    const size_t e1 = (size_t)ne, e2 = 2 * (size_t)ne;
    const size_t grow = 8 * ((m.vals.n < e1 ? e1 : 0) + (m.at.n < e1 ? e1 : 0) + (m.aperm.n < e1 ? e1 : 0) + (m.rhist.n < e2 ? e2 : 0) +
                             (m.rout.n < e2 ? e2 : 0)); // (a buffer that grows is allocated anew)
    if (grow) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b)
            CGE_THROW(CGE_E_OOM, "link_auc: %zu bytes of scratch to allocate for m = %lld edges (56 per edge) do not fit the %zu bytes free",
                      grow, (long long)ne, free_b);
    }
    m.vals.ensure((size_t)ne);
    m.at.ensure((size_t)ne);
    m.aperm.ensure((size_t)ne);
    m.rhist.ensure((size_t)2 * ne);
    m.rout.ensure((size_t)2 * ne);
    m.acnt.ensure(6);
    host_ensure_centred(c);
    k_link_keys(c);
    k_link_prob(c, c->src.p, c->dst.p, ne, m.vals.p);
    k_link_auc(c, part, nparts, m.vals.p, m.at.p, m.aperm.p, m.rhist.p, m.rhist.p + ne, m.acnt.p, m.rout.p, m.rout.p + ne);
    std::vector<int64_t> hl, ht;
    if (!out_less) { hl.resize((size_t)ne); out_less = hl.data(); }
    if (!out_ties) { ht.resize((size_t)ne); out_ties = ht.data(); }
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(out_less, m.rout.p, sizeof(i64) * ne, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(out_ties, m.rout.p + ne, sizeof(i64) * ne, hipMemcpyDeviceToHost, st));
    if (out_p) HIP_CHECK(hipMemcpyAsync(out_p, m.vals.p, sizeof(double) * ne, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(cnt, m.acnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    *n_neg = (m.directed ? n * (n - 1) : n * (n - 1) / 2) - (i64)cnt[5];
    const double *w = c->h_w.empty() ? nullptr : c->h_w.data(); // (no mirror: unit weights)
    long double W = 0.0L, L = 0.0L, Tq = 0.0L;
    for (i64 e = 0; e < ne; e++) {
        const long double we = w ? (long double)w[e] : 1.0L;
        W += we;
        L += we * (long double)out_less[e];
        Tq += we * (long double)out_ties[e];
    }
    summary[0] = (double)W;
    summary[1] = (double)L;
    summary[2] = (double)Tq;
    m.stat_auc_survivors = (i64)cnt[0];
    m.stat_auc_proven = (i64)(cnt[1] + cnt[2]);
    m.stat_auc_tiles = (i64)cnt[4];
    flush_timers(c);
}

// ---- cge_link_moments --------------------------------------------------------------------------------------------------------------
// The host's part: the vertices in community order (a counting sort of the host mirror: stable, ids ascending inside a community),
// the geometry that n alone fixes (blocks of wb x wb tiles, one work item each), per block the communities it meets and per item
// the offset of its bin slots; then one launch and two small ones (kernels_link.hip), the outputs fetched, and the self pairs of
// diag = 1 added here, in vertex order.  Cobs is the sweep's own vect_C pass (host_edge_scatter).
// Scratch on the device, in bytes:  8 dpad ldn  (the operand in community order)  +  16 wb 128 items  (row and column partials;
// items = nB (nB + 1) / 2 undirected, nB^2 directed, nB = ceil(tiles / wb): O(n nB))  +  64 slots  (bin partials, a slot per wave;
// slots = sum over the items of ranks(SI) ranks(SJ) <= (Cp + nB)^2)  +  16 L + 44 n  (outputs, factors, tables).
void host_link_moments(cge_ctx *c, int diag, double *deg_out, double *deg_in, double *B, double *V, double *Cobs, int64_t *n_comm) {
    link_need_inputs(c, "link_moments");
    link_need_model(c, "link_moments");
    if (diag != 0 && diag != 1) CGE_THROW(CGE_E_ARG, "link_moments: diag = %d is neither 0 nor 1", diag);
    LinkModel &m = c->link;
    const i64 n = m.n, C = c->n_comm_max;
    if (!c->comm.p || (i64)c->h_comm.size() != n || C <= 0)
        CGE_THROW(CGE_E_ARG, "link_moments: no resident communities (cge_set_vertex_data)");
    *n_comm = C;
    if (!deg_out && !deg_in && !B && !V && !Cobs) return;
    const int directed = m.directed;
    const i64 L = directed ? C * C : C * (C + 1) / 2;
    hipStream_t st = c->stream;
    // ---- the order and the geometry
    const i64 nT = (n + 127) / 128, wb = k_link_moments_wb(nT), nB = (nT + wb - 1) / wb, bs = wb * 128;
    const i64 items = directed ? nB * nB : nB * (nB + 1) / 2;
    std::vector<i64> start((size_t)C + 1, 0);
    for (i64 v = 0; v < n; v++) start[(size_t)c->h_comm[v] + 1]++;
    i64 Cp = 0;
    for (i64 q = 0; q < C; q++) {
        Cp += start[(size_t)q + 1] > 0;
        start[(size_t)q + 1] += start[(size_t)q];
    }
    // one i32 table: perm (n), rank (n), isi, isj (items each), bfr, bnc (nB each), cid, rb0, rb1 (Cp each)
    const size_t o_perm = 0, o_rank = (size_t)n, o_isi = 2 * (size_t)n, o_isj = o_isi + (size_t)items, o_bfr = o_isj + (size_t)items,
                 o_bnc = o_bfr + (size_t)nB, o_cid = o_bnc + (size_t)nB, o_rb0 = o_cid + (size_t)Cp, o_rb1 = o_rb0 + (size_t)Cp,
                 ntab = o_rb1 + (size_t)Cp;
    std::vector<i32> tab(ntab);
    std::vector<i64> boff((size_t)items);
    {
        std::vector<i64> next(start.begin(), start.end() - 1);
        for (i64 v = 0; v < n; v++) tab[o_perm + (size_t)next[(size_t)c->h_comm[v]]++] = (i32)v;
        i64 r = -1;
        for (i64 q = 0; q < C; q++) {
            if (start[(size_t)q + 1] == start[(size_t)q]) continue;
            r++;
            tab[o_cid + (size_t)r] = (i32)q;
            tab[o_rb0 + (size_t)r] = (i32)(start[(size_t)q] / bs);
            tab[o_rb1 + (size_t)r] = (i32)((start[(size_t)q + 1] - 1) / bs);
            for (i64 p = start[(size_t)q]; p < start[(size_t)q + 1]; p++) tab[o_rank + (size_t)p] = (i32)r;
        }
        for (i64 S = 0; S < nB; S++) {
            const i64 first = tab[o_rank + (size_t)(S * bs)], last = tab[o_rank + (size_t)std::min(n - 1, (S + 1) * bs - 1)];
            tab[o_bfr + (size_t)S] = (i32)first;
            tab[o_bnc + (size_t)S] = (i32)(last - first + 1);
        }
    }
    i64 slots = 0;
    {
        i64 it = 0;
        for (i64 SI = 0; SI < nB; SI++)
            for (i64 SJ = directed ? 0 : SI; SJ < nB; SJ++, it++) {
                tab[o_isi + (size_t)it] = (i32)SI;
                tab[o_isj + (size_t)it] = (i32)SJ;
                boff[(size_t)it] = slots;
                slots += (i64)tab[o_bnc + (size_t)SI] * tab[o_bnc + (size_t)SJ];
            }
    }
    // ---- the scratch
    const size_t nXp = (size_t)c->ldn * (size_t)c->dpad, nrow = 2 * (size_t)items * (size_t)bs, nbin = 8 * (size_t)slots,
                 nout = 2 * (size_t)n + 2 * (size_t)L;
    const size_t grow = 8 * ((m.mXp.n < nXp ? nXp : 0) + (m.mrow.n < nrow ? nrow : 0) + (m.mbin.n < nbin ? nbin : 0) +
                             (m.mout.n < nout ? nout : 0) + (m.mf.n < 2 * (size_t)n ? 2 * (size_t)n : 0));
    if (grow) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b)
            CGE_THROW(CGE_E_OOM,
                      "link_moments: %zu bytes of scratch to allocate (8 dpad ldn + 16 wb 128 items + 64 slots + 16 L + 32 n: wb = %lld, "
                      "items = %lld, slots = %lld, L = %lld) do not fit the %zu bytes free",
                      grow, (long long)wb, (long long)items, (long long)slots, (long long)L, free_b);
    }
    host_ensure_centred(c);
    m.mXp.ensure(nXp);
    m.mrp.ensure((size_t)c->ldn);
    m.mf.ensure(2 * (size_t)n);
    m.mrow.ensure(nrow);
    m.mbin.ensure(nbin);
    m.mout.ensure(nout);
    m.mtab.ensure(ntab);
    m.moff.ensure((size_t)items);
    m.mcnt.ensure(4);
    HIP_CHECK(hipMemcpyAsync(m.mtab.p, tab.data(), sizeof(i32) * ntab, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.moff.p, boff.data(), sizeof(i64) * items, hipMemcpyHostToDevice, st));
    LinkMomentsTables T{};
    T.perm = m.mtab.p + o_perm; T.rank = m.mtab.p + o_rank; T.isi = m.mtab.p + o_isi; T.isj = m.mtab.p + o_isj;
    T.bfr = m.mtab.p + o_bfr; T.bnc = m.mtab.p + o_bnc; T.cid = m.mtab.p + o_cid; T.rb0 = m.mtab.p + o_rb0; T.rb1 = m.mtab.p + o_rb1;
    T.boff = m.moff.p;
    T.wb = wb; T.nT = nT; T.nB = nB; T.items = items; T.slots = slots; T.Cp = Cp; T.C = C;
    double *d_deg = m.mout.p, *d_B = m.mout.p + 2 * n, *d_V = d_B + L;
    k_link_moments(c, T, d_deg, d_B, d_V, L, m.mcnt.p);
    // ---- the outputs
    std::vector<double> h_deg((size_t)(directed ? 2 * n : n)), h_B, h_V, h_f;
    unsigned long long cnt[4] = {0, 0, 0, 0};
    const bool bins = B || V;
    HIP_CHECK(hipMemcpyAsync(h_deg.data(), d_deg, sizeof(double) * h_deg.size(), hipMemcpyDeviceToHost, st));
    if (bins) {
        h_B.resize((size_t)L);
        h_V.resize((size_t)L);
        HIP_CHECK(hipMemcpyAsync(h_B.data(), d_B, sizeof(double) * L, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_V.data(), d_V, sizeof(double) * L, hipMemcpyDeviceToHost, st));
    }
    if (diag) {
        h_f.resize(2 * (size_t)n);
        HIP_CHECK(hipMemcpyAsync(h_f.data(), m.f.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipMemcpyAsync(cnt, m.mcnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st)); // (the host tables above are borrowed by the copies until here)
    i64 sat = (i64)cnt[2];
    if (diag) { // p(i, i) = f_out[i] f_in[i]: once to deg_out (directed: and to deg_in), once to the bin (c_i, c_i), in vertex order
        for (i64 v = 0; v < n; v++) {
            const double p = h_f[(size_t)v] * h_f[(size_t)(n + v)], q = p > 1.0 ? 1.0 : p;
            const i64 q0 = c->h_comm[(size_t)v];
            const i64 at = directed ? q0 * C + q0 : C * q0 - q0 * (q0 - 1) / 2;
            h_deg[(size_t)v] += p;
            if (directed) h_deg[(size_t)(n + v)] += p;
            if (bins) {
                h_B[(size_t)at] += p;
                h_V[(size_t)at] += q * (1.0 - q);
            }
            sat += p > 1.0;
        }
    }
    if (deg_out) std::copy(h_deg.begin(), h_deg.begin() + n, deg_out);
    if (deg_in) std::copy(h_deg.begin() + (directed ? n : 0), h_deg.begin() + (directed ? 2 * n : n), deg_in);
    if (B) std::copy(h_B.begin(), h_B.end(), B);
    if (V) std::copy(h_V.begin(), h_V.end(), V);
    m.stat_mom_exact = (i64)cnt[0];
    m.stat_mom_fast = (i64)cnt[1];
    m.stat_mom_saturated = sat;
    m.stat_mom_tiles = (i64)cnt[3];
    flush_timers(c);
    if (Cobs) host_edge_scatter(c, nullptr, 1, C, directed, 0, c->m, nullptr, Cobs);
}

// ---- cge_link_triangles ------------------------------------------------------------------------------------------------------------
// Model half: Q (8 tld^2 bytes, tld = n padded to an odd number of 128-tiles), the tiles' partials (8 nT^2 128 = tld^2 / 16 bytes at
// most) and two vectors; one generator launch, one triangle launch and its small final, one wedge launch.  Graph half: the sorted
// keys of the model, 24 bytes per edge of oriented keys and long edges, 20 per vertex.  One synchronisation; the four sums are
// taken here in vertex order in long double.
static i64 link_tri_make_q(cge_ctx *c, const char *who, size_t extra_doubles) {
    LinkModel &m = c->link;
    const i64 ld = k_link_tri_ld(m.n);
    const size_t nQ = (size_t)ld * (size_t)ld;
    const size_t grow = 8 * ((m.tQ.n < nQ ? nQ : 0) + extra_doubles);
    if (grow) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b)
            CGE_THROW(CGE_E_OOM, "%s: %zu bytes to allocate for n = %lld (Q: 8 ld^2 with ld = %lld, plus the partials 8 * 128 nT^2) do "
                      "not fit the %zu bytes free", who, grow, (long long)m.n, (long long)ld, free_b);
    }
    m.tQ.ensure(nQ);
    m.tcnt.ensure(2);
    k_link_tri_q(c, m.tQ.p, ld, m.tcnt.p);
    return ld;
}
void host_link_triangles(cge_ctx *c, double *tri_exp, double *wed_exp, int64_t *tri_obs, int64_t *wed_obs, double summary[4]) {
    link_need_inputs(c, "link_triangles");
    link_need_model(c, "link_triangles");
    LinkModel &m = c->link;
    if (m.directed)
        CGE_THROW(CGE_E_ARG, "link_triangles: the model is directed; triangles and wedges are defined for undirected models only");
    const i64 n = m.n, ne = c->m;
    hipStream_t st = c->stream;
    const bool model = tri_exp || wed_exp, graph = tri_obs || wed_obs;
    std::vector<double> h_t, h_w;
    std::vector<unsigned long long> h_tri;
    std::vector<i32> h_deg;
    unsigned long long sat = 0;
    m.stat_tri_tiles = 0;
    m.stat_tri_saturated = 0;
    m.stat_tri_bytes = 0;
    if (model) {
        const i64 nT = (n + 127) / 128;
        const size_t npart = (size_t)nT * (size_t)nT * 128;
        const i64 ld = link_tri_make_q(c, "link_triangles", (m.tpart.n < npart ? npart : 0) + (m.tout.n < 2 * (size_t)n ? 2 * (size_t)n : 0));
        m.tpart.ensure(npart);
        m.tout.ensure(2 * (size_t)n);
        m.stat_tri_tiles = k_link_tri_expected(c, m.tQ.p, ld, m.tpart.p, tri_exp ? m.tout.p : nullptr, wed_exp ? m.tout.p + n : nullptr);
        m.stat_tri_bytes = (i64)(8 * (size_t)ld * (size_t)ld);
        if (tri_exp) {
            h_t.resize((size_t)n);
            HIP_CHECK(hipMemcpyAsync(h_t.data(), m.tout.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        }
        if (wed_exp) {
            h_w.resize((size_t)n);
            HIP_CHECK(hipMemcpyAsync(h_w.data(), m.tout.p + n, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipMemcpyAsync(&sat, m.tcnt.p, sizeof(sat), hipMemcpyDeviceToHost, st));
    }
    if (graph) {
        m.tdeg.ensure((size_t)n);
        m.ttri.ensure((size_t)n);
        m.toff.ensure((size_t)n + 1);
        m.tokeys_in.ensure((size_t)ne);
        m.tokeys.ensure((size_t)ne);
        m.tlong.ensure((size_t)ne);
        m.tcnt.ensure(2);
        k_link_tri_observed(c, m.tdeg.p, m.ttri.p, m.tokeys_in.p, m.tokeys.p, m.toff.p, m.tlong.p, m.tcnt.p + 1);
        h_tri.resize((size_t)n);
        h_deg.resize((size_t)n);
        HIP_CHECK(hipMemcpyAsync(h_tri.data(), m.ttri.p, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(h_deg.data(), m.tdeg.p, sizeof(i32) * n, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    long double S[4] = {0.0L, 0.0L, 0.0L, 0.0L};
    for (i64 v = 0; v < n; v++) {
        if (tri_exp) S[0] += (long double)(tri_exp[v] = h_t[(size_t)v]);
        if (wed_exp) S[1] += (long double)(wed_exp[v] = h_w[(size_t)v]);
        if (graph) {
            const i64 k = h_deg[(size_t)v], t = (i64)h_tri[(size_t)v], w = k * (k - 1) / 2;
            if (tri_obs) tri_obs[v] = t;
            if (wed_obs) wed_obs[v] = w;
            S[2] += (long double)t;
            S[3] += (long double)w;
        }
    }
    for (int q = 0; q < 4; q++) summary[q] = (double)S[q];
    m.stat_tri_saturated = (i64)sat;
    flush_timers(c);
}
void host_link_triangles_q(cge_ctx *c, double *Q_out, i64 ld) {
    link_need_inputs(c, "link_triangles_test");
    link_need_model(c, "link_triangles_test");
    LinkModel &m = c->link;
    if (m.directed) CGE_THROW(CGE_E_ARG, "link_triangles_test: the model is directed; undirected models only");
    if (m.n > 2048) CGE_THROW(CGE_E_ARG, "link_triangles_test: n = %lld is beyond the hook's 2048 vertices", (long long)m.n);
    const i64 ldq = k_link_tri_ld(m.n);
    if (ld != ldq)
        CGE_THROW(CGE_E_ARG, "link_triangles_test: ld = %lld, Q of n = %lld has leading dimension %lld", (long long)ld, (long long)m.n,
                  (long long)ldq);
    link_tri_make_q(c, "link_triangles_test", 0);
    HIP_CHECK(hipMemcpyAsync(Q_out, m.tQ.p, sizeof(double) * ldq * ldq, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    flush_timers(c);
}
