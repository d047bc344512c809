// batch_host.cpp -- the alpha sweeps of cge_score_batch's launch groups in lock-step ("Scoring several embeddings").
// Every member of a group was prepared by host_wgcl_sweep on the fused path and handed over (SweepHandoff).  An alpha of the group
// is three launches for all its live members -- fit_flow_multi_kernel (the members' fused fits side by side), bvec_bins_multi_kernel
// and the two JS kernels with the member in blockIdx.y -- and one copy of the members' scalars to the host.  Per member the host
// keeps what host_wgcl_sweep keeps: its T rotating through three vectors and its alpha bookkeeping (AlphaBook: the patience
// counters of src/divergence.jl:215-223, :242-253, the partial sums added in block order).  So a member's iterates, iteration
// counts and scores are those of its own cge_score.
// A group of DIRECTED members (hand_off_directed) shares the fit alone: fit_flow_dir_multi_kernel between the members' own
// power-matrix launches and their own tallies / vect_B / JS launches, without look-ahead (host_batch_sweep_dir).
#include <algorithm>
#include <cstring>

#include "common.hpp"

bool batch_group_closes(int g_sum, int g_nw, int g_size, int G, int NW, int cus) {
    return g_size > 0 && (g_sum + G > cus || NW != g_nw || g_size >= CGE_BATCH_MAX);
}

// A directed group (members handed over by hand_off_directed).  An alpha: (1) every live member's power matrix into its own GD,
// (2) ONE fit_flow_dir_multi_kernel launch for all of them, (3) per member the launches its own enqueue_alpha makes behind the
// fit -- the local score's tallies, k_bvec in the form its sweep picked, k_js -- on the context's scratch, one member after the
// other on the one stream, (4) one copy of the members' scalars to the pinned slot and an event.  Tin / Tout are updated in
// place, so -- host_wgcl_sweep's own rule for directed sweeps -- the next alpha is not enqueued before this one's verdicts.
static void host_batch_sweep_dir(cge_ctx *c, std::vector<BatchMember *> &group) {
    const i64 n_alpha = AlphaBook::n_alpha;
    const int K = (int)group.size();
    hipStream_t st = c->stream;
    const int NW = group[0]->h.geo.NW;
    c->batch_scal.ensure((size_t)K * RES_STRIDE);
    c->batch_pin.ensure((size_t)2 * K * RES_STRIDE);
    double *scal = c->batch_scal.p;
    std::vector<AlphaBook> book;
    std::vector<char> done(K, 0);
    for (int j = 0; j < K; j++) {
        const SweepHandoff &h = group[j]->h;
        book.emplace_back(h.S, h.split, group[j]->trace);
        c->sw_rowbins.ensure((size_t)h.N * h.C); // the scratch stage 3 lends every member
        c->sw_vectB.ensure((size_t)h.C * h.C);
    }
    for (i64 ia = 1; ia <= n_alpha; ia++) {
        std::vector<int> A;
        for (int j = 0; j < K; j++)
            if (!done[j] && !group[j]->redo) A.push_back(j);
        if (A.empty()) break;
        const double alpha = AlphaBook::AlphaStep * (double)ia;
        cge_flow_dir_multi tab{};
        tab.n = (int)A.size();
        for (int i = 0; i < (int)A.size(); i++) {
            SweepHandoff &h = group[A[i]]->h;
            k_pow_matrix_from(c, h.D.p, h.logs ? h.Lh.p : nullptr, h.logs ? h.Ll.p : nullptr, h.N, alpha, h.GD.p, false);
            cge_flow_dir_problem &q = tab.p[i];
            q.GD = h.GD.p;
            q.Tin = h.Tio.p; q.Tout = h.Tio.p + h.N;
            q.deg_in = h.deg.p; q.deg_out = h.deg.p + h.N;
            q.flags = reinterpret_cast<int *>(scal + (i64)A[i] * RES_STRIDE + RES_FIT);
            q.N = h.N; q.Tld = h.Tld; q.Nt = h.geo.Nt; q.G = h.geo.G;
        }
        k_fit_flow_dir_multi(c, tab, NW, 0.9, 1.0, AlphaBook::delta, c->batch_flow); // epsilon, diff (:434-435)
        c->stat_fit_batched_launches++;
        for (int j : A) {
            SweepHandoff &h = group[j]->h;
            double *sj = scal + (i64)j * RES_STRIDE;
            const double *Ta = h.Tio.p + h.N, *Tb = h.Tio.p; // (Tout, Tin), as enqueue_alpha names them
            const DevSamples &ds = *h.dsets[h.n_sets == 1 ? 0 : ia - 1];
            if (!book[j].skip_auc)
                k_auc_landmark(c, Ta, Tb, h.v2l.p, c->vw.p, h.lweight.p, ds.pi.p, ds.pj.p, ds.ni.p, ds.nj.p, ds.dpos.p, ds.dneg.p,
                               ds.wts.p, h.S, alpha, nullptr, sj + RES_AUC);
            if (!book[j].skip_div) {
                double *vB = c->sw_vectB.p;
                k_bvec(c, h.GD.p, Ta, Tb, h.cm_pos.p, h.cm_off.p, h.cm_mem.p, h.N, h.C, 1, c->sw_rowbins.p, vB, h.bvec_form);
                if (!h.split)
                    k_js(c, h.vectC.p, vB, h.C * h.C, h.C, 1, 0, nullptr, sj + RES_JS);
                else {
                    k_js(c, h.vectC.p, vB, h.C * h.C, h.C, 1, 1, nullptr, sj + RES_JS);
                    k_js(c, h.vectC.p, vB, h.C * h.C, h.C, 1, 2, nullptr, sj + RES_JS + CGE_PARTIAL_BLOCKS);
                }
            }
        }
        const int slot = (int)(ia & 1);
        HIP_CHECK(hipMemcpyAsync(c->batch_pin.p + (i64)slot * K * RES_STRIDE, scal, sizeof(double) * K * RES_STRIDE,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipEventRecord(c->sweep_ev[slot], st));
        HIP_CHECK(hipEventSynchronize(c->sweep_ev[slot]));
        for (int j : A) {
            BatchMember &mb = *group[j];
            const double *res = c->batch_pin.p + (i64)slot * K * RES_STRIDE + (i64)j * RES_STRIDE;
            const int *hf = reinterpret_cast<const int *>(res + RES_FIT);
            if (hf[2] || !hf[0]) { // abandoned (Tin / Tout untouched): the member is scored again on its own
                note_fit_fallback(c);
                mb.redo = true;
                continue;
            }
            c->stat_fit_batched_alphas++;
            book[j].take(res, alpha, hf[1]);
            if (book[j].ended() || ia == n_alpha) {
                done[j] = 1;
                book[j].write(mb.out, mb.out_len);
            }
        }
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (c->stat_fit_batched_alphas > 0 && !c->fit_persistent_broken) c->fit_fallback_streak = 0; // clean persistent sweeps
}

void host_batch_sweep(cge_ctx *c, std::vector<BatchMember *> &group) {
    const i64 n_alpha = AlphaBook::n_alpha;
    const int K = (int)group.size();
    if (K < 1) return;
    if (group[0]->h.directed) return host_batch_sweep_dir(c, group);
    hipStream_t st = c->stream;
    const int NW = group[0]->h.geo.NW;
    i64 vtot = 0;
    std::vector<i64> voff(K);
    for (int j = 0; j < K; j++) {
        voff[j] = vtot;
        vtot += packed_len(group[j]->h.C);
    }
    c->batch_scal.ensure((size_t)K * RES_STRIDE);
    c->batch_vectB.ensure((size_t)vtot);
    c->batch_jspart.ensure((size_t)2 * K * 3 * CGE_PARTIAL_BLOCKS);
    c->batch_pin.ensure((size_t)2 * K * RES_STRIDE);
    double *scal = c->batch_scal.p; // the members' scalars of an alpha (RES_*), RES_STRIDE apart

    struct Live {
        int tpar = 0;         // the part of T that holds the current iterate
        i64 next_enqueue = 1; // the next alpha to enqueue
        DevBuf<char> epi;     // the epilogue tables with the tallies pointed at this member's scalars
        bool done = false;
    };
    std::vector<Live> live(K);
    std::vector<AlphaBook> book;
    for (int j = 0; j < K; j++) {
        SweepHandoff &h = group[j]->h;
        std::vector<cge_fit_fused> e = h.h_epi;
        for (cge_fit_fused &f : e) f.auc_part = scal + (i64)j * RES_STRIDE + RES_AUC;
        live[j].epi.ensure(e.size() * sizeof(cge_fit_fused));
        HIP_CHECK(hipMemcpyAsync(live[j].epi.p, e.data(), e.size() * sizeof(cge_fit_fused), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st)); // (pageable source)
        book.emplace_back(h.S, h.split, group[j]->trace);
    }
    auto running = [&](int j) { return !live[j].done && !group[j]->redo; };

    // one alpha for the members in `A`: the fits, vect_B, JS, the scalars to pinned slot (ia & 1), an event
    auto enqueue = [&](i64 ia, const std::vector<int> &A) {
        if (A.empty()) return;
        const double alpha = AlphaBook::AlphaStep * (double)ia;
        cge_flow_multi tab{};
        cge_bins_multi bins{};
        cge_js_multi js{};
        int nb = 0, nj = 0;
        i64 maxC = 0;
        tab.n = (int)A.size();
        for (int i = 0; i < (int)A.size(); i++) {
            const int j = A[i];
            Live &L = live[j];
            SweepHandoff &h = group[j]->h;
            const bool want_auc = !book[j].skip_auc, want_div = !book[j].skip_div;
            const int Nt = h.geo.Nt, tnext = (L.tpar + 1) % 3;
            double *sj = scal + (i64)j * RES_STRIDE;
            tab.p[i] = flow_problem_entry(h.Lh.p, h.Ll.p, alpha,
                                          reinterpret_cast<const cge_fit_fused *>(L.epi.p) + (h.n_sets == 1 ? 0 : ia - 1),
                                          (want_div ? 1 : 0) | (want_auc ? 2 : 0), h.T.p + (i64)L.tpar * h.Tld,
                                          h.T.p + (i64)tnext * h.Tld, h.w, reinterpret_cast<int *>(sj + RES_FIT), h.N, h.Tld, h.geo);
            L.tpar = tnext;
            L.next_enqueue = ia + 1;
            if (!want_div) continue;
            double *vB = c->batch_vectB.p + voff[j];
            bins.p[nb++] = cge_bins_problem{h.bt_part.p, h.cm_off.p, h.bt_fc.p, h.bt_ns.p, h.bt_base.p, h.C, Nt, 0, vB};
            maxC = std::max(maxC, h.C);
            const int modes[2] = {h.split ? 1 : 0, 2};
            for (int u = 0; u < (h.split ? 2 : 1); u++, nj++)
                js.p[nj] = cge_js_problem{h.vectC.p, vB, packed_len(h.C), h.C, modes[u], 0,
                                          c->batch_jspart.p + (i64)nj * 3 * CGE_PARTIAL_BLOCKS, sj + RES_JS + u * CGE_PARTIAL_BLOCKS};
        }
        k_fit_flow_multi(c, tab, NW, 0.25, AlphaBook::delta, c->batch_flow);
        c->stat_fit_batched_launches++;
        k_bins_js_multi(c, bins, nb, maxC, js, nj);
        const int slot = (int)(ia & 1);
        HIP_CHECK(hipMemcpyAsync(c->batch_pin.p + (i64)slot * K * RES_STRIDE, scal, sizeof(double) * K * RES_STRIDE,
                                 hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipEventRecord(c->sweep_ev[slot], st));
    };

    for (i64 ia = 1; ia <= n_alpha; ia++) {
        std::vector<int> A, B;
        for (int j = 0; j < K; j++)
            if (running(j) && live[j].next_enqueue == ia) A.push_back(j);
        enqueue(ia, A);
        // the next alpha of every member that cannot end at this one is enqueued before the host waits (host_wgcl_sweep's overlap)
        bool any = false;
        for (int j = 0; j < K; j++) {
            if (!running(j)) continue;
            any = true;
            if (!book[j].may_end_here() && ia < n_alpha && live[j].next_enqueue == ia + 1) B.push_back(j);
        }
        if (!any) break;
        enqueue(ia + 1, B);
        HIP_CHECK(hipEventSynchronize(c->sweep_ev[ia & 1]));
        for (int j = 0; j < K; j++) {
            if (!running(j)) continue;
            BatchMember &mb = *group[j];
            const double *res = c->batch_pin.p + (i64)(ia & 1) * K * RES_STRIDE + (i64)j * RES_STRIDE;
            const int *hf = reinterpret_cast<const int *>(res + RES_FIT);
            if (hf[2] || !hf[0]) { // abandoned (a wait timed out): the member is scored again on its own
                note_fit_fallback(c);
                mb.redo = true;
                continue;
            }
            c->stat_fit_batched_alphas++;
            book[j].take(res, AlphaBook::AlphaStep * (double)ia, hf[1]);
            if (book[j].ended() || ia == n_alpha) {
                live[j].done = true;
                book[j].write(mb.out, mb.out_len);
            }
        }
    }
    HIP_CHECK(hipStreamSynchronize(st)); // (an alpha enqueued ahead for a member that then stopped: nothing reads it)
    if (c->stat_fit_batched_alphas > 0 && !c->fit_persistent_broken) c->fit_fallback_streak = 0; // clean persistent sweeps
}

// ---- cge_score_batch: K embeddings of the resident graph ("Scoring several embeddings") ----------------------------
// A member is a cge_embedding_view (cge_score_batch describes its fp64 matrices as views); `who` names the entry point in messages.
static void upload_member(cge_ctx *c, const char *who, const cge_embedding_view *views, i64 k) {
    try {
        set_embedding_view(c, "set_embedding_view", views + k, c->n);
    } catch (const CgeError &e) {
        CGE_THROW(e.code, "%s: embedding %lld: %s", who, (long long)k, e.msg.c_str());
    } catch (const std::bad_alloc &) { // (with the text and the codes of the boundary, CGE_CATCH)
        CGE_THROW(CGE_E_OOM, "%s: embedding %lld: host allocation failed", who, (long long)k);
    } catch (const std::exception &e) {
        CGE_THROW(CGE_E_ARG, "%s: embedding %lld: %s", who, (long long)k, e.what());
    }
}
static void score_batch_impl(cge_ctx *c, const cge_score_args *a, const cge_embedding_view *views, i64 K, const char *who, double *out,
                             int *out_len, cge_trace *traces) {
    if (!c->src.p || !c->vw.p || !c->comm.p || c->n <= 0 || c->m <= 0)
        CGE_THROW(CGE_E_ARG, "%s: graph and vertex data must be resident (cge_set_graph / cge_set_vertex_data)", who);
    if (c->has_coll || c->rccl_comm || c->edges_sharded || c->rows_sharded || c->opt_shard_ingest || c->opt_shard_rows)
        CGE_THROW(CGE_E_ARG, "%s: not under collectives or sharding (one embedding per rank is the multi-GPU form)", who);
    for (i64 k = 0; k < K; k++) { // the members, before any work
        std::string msg;
        if (view_check(views + k, c->n, msg) != CGE_OK) CGE_THROW(CGE_E_ARG, "%s: embedding %lld: %s", who, (long long)k, msg.c_str());
        if (views[k].on_device) check_device_pointer(c, (std::string(who) + ": embedding " + std::to_string(k)).c_str(), views[k].data);
    }
    const int cus = device_cus(c);
    // the members that can take the batched sweep (landmark mode; undirected: the fused fit, directed: the persistent fit of >= 256
    // landmarks); the sweep decides the rest
    // (one member, or a member whose fit takes more than half the chip, shares nothing: it is scored as cge_score scores it)
    // (directed members: the shared directed fit, which has no fused chain -- option fit_fused does not apply to them)
    const bool batchable = K >= 2 && a->land != -1 && c->opt_fit_persistent != 1 &&
                           (a->directed ? !c->fit_persistent_broken : c->opt_fit_fused != 0);
    c->stat_fit_batched_launches = c->stat_fit_batched_alphas = 0;
    c->smp.reset();
    bool have_samples = false;
    std::vector<std::unique_ptr<BatchMember>> group;
    std::vector<i64> redo, group_k;
    int g_sum = 0, g_nw = 0;
    double batch_ms = 0.0;
    auto run_group = [&]() {
        if (group.empty()) return;
        std::vector<BatchMember *> g;
        for (auto &m : group) g.push_back(m.get());
        const double t0 = now_ms();
        host_batch_sweep(c, g);
        batch_ms += now_ms() - t0;
        for (size_t i = 0; i < group.size(); i++)
            if (group[i]->redo) redo.push_back(group_k[i]);
        group.clear(); group_k.clear();
        g_sum = 0;
    };
    for (i64 k = 0; k < K; k++) {
        upload_member(c, who, views, k);
        std::unique_ptr<BatchMember> m(new BatchMember());
        m->h.max_G = cus / 2;
        m->out = out + 7 * k; m->out_len = out_len + k; m->trace = traces ? traces + k : nullptr;
        host_score(c, a, m->out, m->out_len, m->trace, batchable ? &m->h : nullptr, have_samples);
        have_samples = have_samples || c->smp.n_sets > 0;
        if (!m->h.deferred) continue; // (scored: the sequential path)
        if (batch_group_closes(g_sum, g_nw, (int)group.size(), m->h.geo.G, m->h.geo.NW, cus)) run_group();
        g_sum += m->h.geo.G;
        g_nw = m->h.geo.NW;
        group.push_back(std::move(m));
        group_k.push_back(k);
    }
    run_group();
    flush_timers(c);
    // members whose batched fit was abandoned: cge_score's own path (which falls back to one launch per iteration as it must)
    std::sort(redo.begin(), redo.end());
    for (i64 k : redo) {
        upload_member(c, who, views, k);
        host_score(c, a, out + 7 * k, out_len + k, traces ? traces + k : nullptr, nullptr, true);
    }
    if (!redo.empty() && redo.back() != K - 1) { // the resident embedding and landmark state are the last member's
        upload_member(c, who, views, K - 1);
        host_landmarks_run(c, score_landmark_run(c, a));
    }
    c->phases.ms["batch_sweep"] = batch_ms; // the launch groups' sweeps, all members (the other phases: the last member's)
}
// the boundary of both batch entry points: every exit leaves the context usable, an error leaves every out_len at 0
int score_batch_run(cge_ctx *c, const cge_score_args *a, const cge_embedding_view *views, i64 K, const char *who, double *out,
                    int *out_len, cge_trace *traces) {
    for (i64 k = 0; k < K; k++) out_len[k] = 0;
    const int rc = [&]() -> int {
        CGE_TRY_ON_DEVICE(c)
        score_batch_impl(c, a, views, K, who, out, out_len, traces);
        CGE_CATCH(c)
    }();
    // on every exit: no hand-off slot taken for armed (host_score leaves no pending sample draw behind)
    c->flow_armed_words = 0;
    if (rc != CGE_OK) {
        (void)hipStreamSynchronize(c->stream);
        for (i64 k = 0; k < K; k++) out_len[k] = 0;
    }
    return rc;
}
