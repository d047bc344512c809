// sweep_hooks.cpp -- the kernel-level testing hooks of the alpha sweep (include/cge_hip_testing.h): each runs the sweep's own
// functions (sweep_internal.hpp) and launch wrappers on a caller's problem.  No cge_score runs anything in this file.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sweep_internal.hpp"
#include "../../include/cge_hip_testing.h"

// ---- what the hooks stage alike ------------------------------------------------------------------------------------------

// host <-> device copies on the context's stream (down: a NULL host pointer is not copied)
template <class T>
static void hook_up(cge_ctx *c, DevBuf<T> &dev, const T *host, i64 cnt) {
    dev.ensure((size_t)cnt);
    HIP_CHECK(hipMemcpyAsync(dev.p, host, sizeof(T) * cnt, hipMemcpyHostToDevice, c->stream));
}
template <class T> // two host arrays in one buffer, the second behind the first
static void hook_up2(cge_ctx *c, DevBuf<T> &dev, const T *a, i64 na, const T *b, i64 nb) {
    dev.ensure((size_t)(na + nb));
    HIP_CHECK(hipMemcpyAsync(dev.p, a, sizeof(T) * na, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(dev.p + na, b, sizeof(T) * nb, hipMemcpyHostToDevice, c->stream));
}
template <class T>
static void hook_down(cge_ctx *c, T *host, const T *dev, i64 cnt) {
    if (host) HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(T) * cnt, hipMemcpyDeviceToHost, c->stream));
}
// all bits set: a NaN in every double or float, where nothing may write or until something does
static void fill_nan(cge_ctx *c, void *dev, size_t bytes) { HIP_CHECK(hipMemsetAsync(dev, 0xFF, bytes, c->stream)); }

namespace {
// the options that choose vect_B's form and decide whether a layout is the fused one, as a hook sets them; restored on the way out
struct HookOptions {
    cge_ctx *c;
    const int blocks = c->opt_bvec_blocks, plain = c->opt_test_bvec_plain, fused = c->opt_fit_fused, persistent = c->opt_fit_persistent;
    const bool relabel = c->opt_exact_relabel;
    ~HookOptions() {
        c->opt_bvec_blocks = blocks; c->opt_test_bvec_plain = plain; c->opt_fit_fused = fused;
        c->opt_fit_persistent = persistent; c->opt_exact_relabel = relabel;
    }
};
} // namespace

// a caller's community ids (1 .. C), checked and 0-based
template <class Id>
static std::vector<i32> hook_comm0(const char *who, const Id *comm1, i64 N, i64 C) {
    std::vector<i32> hcomm(N);
    for (i64 i = 0; i < N; i++) {
        if (comm1[i] < 1 || comm1[i] > C) CGE_THROW(CGE_E_ARG, "%s: community id out of range", who);
        hcomm[i] = (i32)(comm1[i] - 1);
    }
    return hcomm;
}

// The device tables of a layout as a sweep stages them: community_tables and -- not on every call: under the sweep's own condition,
// the tiles apply and the problem is undirected -- k_bins_prepare.  A hook calls layout_tables itself, states its own refusals of
// the layout, which come before anything is launched, and reads the layout's order (lay.cm_mem: the caller's vertex at each position
// of the sweep's numbering) before this call -- the sweep computes GD from permuted rows, so a relabelled hook permutes its host
// arrays by it (hook_permuted).
static void hook_layout_tables(cge_ctx *c, SweepLayout &lay, i64 N, i64 C, int directed) {
    if (lay.relabel)
        for (i64 q = 0; q < N; q++) lay.cm_mem[q] = (i32)q; // the member lists in the new numbering, as plan_layout leaves them
    WordPacker pk(c);
    std::vector<i32> cm_pos;
    community_tables(c, lay, N, C, pk, cm_pos);
    pk.flush();
    if (c->bvec_blocks && !directed) k_bins_prepare(c, c->sw_cm_off.p, N, C, lay.bt_total);
}
// a caller's vector (square: matrix, its columns too) in the sweep's numbering: row q is the caller's row order[q]
static std::vector<double> hook_permuted(const std::vector<i32> &order, const double *x, bool square) {
    const i64 N = (i64)order.size(), W = square ? N : 1;
    std::vector<double> out((size_t)N * W);
    for (i64 q = 0; q < N; q++)
        for (i64 r = 0; r < W; r++) out[q * W + r] = x[order[q] * W + (square ? order[r] : 0)];
    return out;
}

// the upper 64 x 64 tiles of a host matrix, zeros outside the matrix, through the address inline every consumer uses, in sw_PK
static void pack_upper_tiles(cge_ctx *c, const double *M, i64 N) {
    const i64 Nt = (N + 63) / 64;
    std::vector<double> pk((size_t)(Nt * (Nt + 1) / 2) * CGE_TILE_DOUBLES, 0.0);
    for (i64 i = 0; i < N; i++)
        for (i64 j = i / 64 * 64; j < N; j++) pk[cge_packed_index(i, j, Nt)] = M[i * N + j];
    hook_up(c, c->sw_PK, pk.data(), (i64)pk.size());
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (pk goes out of scope)
}

// one member's entries of a bins / JS launch's table, from js.p[nj] on: mode 0, or (n_modes = 2) modes 1 and 2; entry u takes the
// u-th 3 * CGE_PARTIAL_BLOCKS doubles of `part` and the u-th CGE_PARTIAL_BLOCKS of `fpart`
static void hook_js_entries(cge_js_multi &js, int &nj, const double *vC, const double *vB, i64 len, i64 C, int n_modes, double *part,
                            double *fpart) {
    for (int u = 0; u < n_modes; u++, nj++)
        js.p[nj] = cge_js_problem{vC, vB, len, C, n_modes == 1 ? 0 : 1 + u, 0, part + (i64)u * 3 * CGE_PARTIAL_BLOCKS,
                                  fpart + (i64)u * CGE_PARTIAL_BLOCKS};
}

// ---- the testing hook of vect_B (include/cge_hip_testing.h: cge_vect_b_test) ------------------------------------------

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
    SweepLayout lay;
    layout_tables(c, hook_comm0("vect_b_test", p.comm, N, C).data(), N, C, directed, form == 0 && landmarks, form == 3, lay);
    if (form >= 4 && !c->bvec_blocks)
        CGE_THROW(CGE_E_ARG, "vect_b_test: the tiles decline this layout (more than 64 community ids in a 64-vertex block)");
    const int run = form != 0 ? form : (c->bvec_blocks && !directed && !c->opt_test_bvec_plain) ? 5 : k_bvec_form(c, N);
    c->sw_rowbins.ensure((size_t)N * C);
    std::vector<double> hGD, hTa, hTb; // (relabelled) in the sweep's numbering
    if (lay.relabel) {
        hTa = hook_permuted(lay.cm_mem, p.Ta, false);
        hTb = hook_permuted(lay.cm_mem, p.Tb, false);
        if (directed) hGD = hook_permuted(lay.cm_mem, p.GD, true);
        else { // the caller's upper triangle is the matrix
            hGD.resize((size_t)N * N);
            for (i64 q = 0; q < N; q++)
                for (i64 r = 0; r < N; r++) {
                    const i64 a = lay.cm_mem[q], b = lay.cm_mem[r];
                    hGD[q * N + r] = a <= b ? p.GD[a * N + b] : p.GD[b * N + a];
                }
        }
    }
    hook_up(c, c->sw_GD, lay.relabel ? hGD.data() : p.GD, N * N);
    hook_up(c, c->sw_T1, lay.relabel ? hTa.data() : p.Ta, N);
    hook_up(c, c->sw_T2, lay.relabel ? hTb.data() : p.Tb, N);
    hook_layout_tables(c, lay, N, C, directed);
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (the host copies go out of scope)
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
    if (form == 7 && !directed) CGE_THROW(CGE_E_ARG, "vect_b_test: form 7 is directed only");
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
    HookOptions restore{c};
    const i64 G = CGE_VECT_B_GUARD;
    const i64 len[2] = {vb_len(p1->C, directed), probs[1] ? vb_len(probs[1]->C, directed) : 0};
    const i64 off[2] = {0, len[0] + G};
    // both vectors back to back, each followed by a guard of NaNs that nothing may write
    std::vector<double> hv((size_t)(len[0] + len[1] + 2 * G), std::nan(""));
    if (!p1->GD) std::memcpy(hv.data(), p1->vectB, sizeof(double) * len[0]);
    DevBuf<double> vB, vC, fpart, part, jsd;
    hook_up(c, vB, hv.data(), (i64)hv.size());
    { // vect_C of both problems (zeros where the caller has none and the form reads one)
        std::vector<double> hc((size_t)(len[0] + len[1]), 0.0);
        for (int q = 0; q < 2; q++)
            if (probs[q] && probs[q]->vC) std::memcpy(hc.data() + (q ? len[0] : 0), probs[q]->vC, sizeof(double) * len[q]);
        hook_up(c, vC, hc.data(), (i64)hc.size());
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
        } else if (run == 7) { // directed, on the packed tiles: the stored tiles and their mirrors, then the bins
            std::vector<double> h((size_t)N * N);
            hook_down(c, h.data(), c->sw_GD.p, N * N); // (in the sweep's numbering)
            HIP_CHECK(hipStreamSynchronize(st));
            pack_upper_tiles(c, h.data(), N);
            k_bvec_tiles(c, c->sw_PK.p, c->sw_T1.p, c->sw_T2.p, c->sw_cm_off.p, N, 1, true);
            k_bvec_bins(c, c->sw_cm_off.p, N, C, 1, vB.p);
            HIP_CHECK(hipStreamSynchronize(st));
            c->sw_PK.release(); // (held only while packed sweeps run)
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
            hook_js_entries(js, nj, vCp[q], vB.p + off[q], len[q], probs[q]->C, nm, part.p + (i64)nj * 3 * CGE_PARTIAL_BLOCKS,
                            fpart.p + (i64)nj * CGE_PARTIAL_BLOCKS);
        k_bins_js_multi(c, bins, 2, p1->C, js, nj);
        HIP_CHECK(hipStreamSynchronize(st)); // (the first problem's tables are released below)
    }
    *form_ran = run;
    std::vector<double> hf((size_t)4 * CGE_PARTIAL_BLOCKS, 0.0);
    if (run == 5 || run == 6) hook_down(c, hf.data(), fpart.p, (i64)hf.size());
    // k_js modes 0, 1, 2 over the vector(s) the form left
    jsd.ensure(6);
    double hj[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 2; q++)
        if (probs[q] && probs[q]->vC)
            for (int mode = 0; mode < 3; mode++)
                k_js(c, vCp[q], vB.p + off[q], len[q], probs[q]->C, directed, mode, jsd.p + 3 * q + mode);
    hook_down(c, hj, jsd.p, 6);
    hook_down(c, hv.data(), vB.p, (i64)hv.size());
    HIP_CHECK(hipStreamSynchronize(st));
    for (int q = 0; q < 2; q++) {
        const cge_vect_b_problem *p = probs[q];
        if (!p) continue;
        if (p->GD) std::memcpy(p->vectB, hv.data() + off[q], sizeof(double) * (len[q] + G));
        if (p->vC) std::memcpy(p->js_dev, hj + 3 * q, sizeof(double) * 3);
        if (p->js_fused && (run == 5 || run == 6))
            for (int u = 0; u < nm; u++) p->js_fused[u] = vb_fold(hf.data() + (i64)((run == 6 ? q * nm : 0) + u) * CGE_PARTIAL_BLOCKS);
    }
}

// ---- the testing hook of the Chung-Lu fit (include/cge_hip_testing.h: cge_fit_test) -------------------------------------------
// One fit from a caller's start through fit_undirected / fit_directed (forms 0-4), k_fit_flow_multi (form 5) or
// k_fit_flow_dir_multi (form 6), on the buffers a sweep keeps them in.  Everything that can refuse does so before the first launch.

// D to sw_D and, when the form or the caller reads it, GD = (1 - D)^alpha to sw_GD by the sweep's two launches (upper: the upper
// tiles alone, as a landmark-mode sweep makes it; everything else of sw_GD is NaN) and to the caller's GD; blocked: behind them the
// tile-blocked logarithm of D, which a fused fit makes its power matrix from
static void ft_matrices(cge_ctx *c, const cge_fit_problem &p, bool upper, bool need_gd, bool blocked = false) {
    const i64 N = p.N;
    hook_up(c, c->sw_D, p.D, N * N);
    if (need_gd || p.GD) {
        c->sw_GD.ensure((size_t)N * N);
        fill_nan(c, c->sw_GD.p, sizeof(double) * N * N);
        k_pow_prepare(c, c->sw_D.p, N, upper);
        k_pow_matrix(c, c->sw_D.p, N, p.alpha, c->sw_GD.p, upper);
        hook_down(c, p.GD, c->sw_GD.p, N * N);
    }
    if (blocked) k_pow_prepare(c, c->sw_D.p, N, true, true);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
// A fit's start on the device: T_0 in part 0 of a T of `parts` parts of Tld doubles (zero beyond N), NaN in the rows of the other
// parts, and the weights
static void ft_start(cge_ctx *c, const cge_fit_problem &p, double *T, int parts, i64 Tld, DevBuf<double> &w) {
    const std::vector<double> nan_n(p.N, std::nan(""));
    HIP_CHECK(hipMemsetAsync(T, 0, sizeof(double) * parts * Tld, c->stream));
    HIP_CHECK(hipMemcpyAsync(T, p.T0, sizeof(double) * p.N, hipMemcpyHostToDevice, c->stream));
    for (int k = 1; k < parts; k++)
        HIP_CHECK(hipMemcpyAsync(T + k * Tld, nan_n.data(), sizeof(double) * p.N, hipMemcpyHostToDevice, c->stream));
    hook_up(c, w, p.w, p.N);
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (nan_n goes out of scope)
}

// the verdict of an enqueued persistent fit: flags [0] converged, [1] iterations, [2] abandoned
static bool ft_verdict(cge_ctx *c, const int *dev_flags, i64 *iters) {
    int hf[4];
    HIP_CHECK(hipMemcpyAsync(hf, dev_flags, sizeof(hf), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    *iters = hf[1];
    return !(hf[2] || !hf[0]);
}

// One fit through `run_fit(sl)` (fit_undirected / fit_directed on the staged problem) and its verdict: an abandoned persistent fit
// is, at form 0, redone as the sweep redoes it -- again from T_0 with one launch (pair) per iteration -- and is status 1 at a forced
// form; a forced persistent form that was declined throws.  Returns the form that ran.
template <class Fit>
static int ft_run(cge_ctx *c, cge_fit_problem &p, int form, int directed, double eps, double delta, FitForm &fit, Fit run_fit) {
    fit.eps = eps;
    fit.delta = delta;
    (directed ? fit.persistent_dir : fit.persistent) = form == 3 || form == 4 || (form == 0 && persistent_wanted(c, p.N));
    AlphaSlot sl;
    run_fit(sl);
    int ran = form == 2 || form == 7 || form == 8 ? form : 1;
    p.status = 0;
    if (sl.fit_async) {
        ran = form == 4 ? 4 : 3;
        if (!ft_verdict(c, (const int *)(c->sw_scal.p + RES_FIT), &sl.iters)) {
            if (form == 0) {
                leave_persistent(c, directed, fit, sl);
                sl = AlphaSlot();
                run_fit(sl);
                ran = 1;
            } else
                p.status = 1;
        }
    } else if (form == 3 || form == 4)
        CGE_THROW(CGE_E_ASSERT, "fit_test: the persistent launch of form %d was declined (N = %lld)", form, (long long)p.N);
    p.iters = sl.iters;
    return ran;
}

// epi (form 4, the hooks of the local score and of the fused chain): the host copy of the epilogue's table, whose device copy is
// the context's (fused_tables, fused_upload); the launch then wants of the epilogue what epi_want names (bit 0 vect_B's tile partials, bit 1 the tally), as
// enqueue_alpha leaves out what an alpha does not want -- the local score's hook the tally alone.
static int ft_undirected(cge_ctx *c, cge_fit_problem &p, int form, double eps, double delta, const cge_fit_fused *epi = nullptr,
                         int epi_want = 2) {
    hipStream_t st = c->stream;
    const i64 N = p.N, Nt = (N + 63) / 64, Tld = Nt * 64;
    ft_matrices(c, p, true, form != 4, form == 4);
    if (form == 2) { // the upper tiles of GD
        std::vector<double> h((size_t)N * N);
        hook_down(c, h.data(), c->sw_GD.p, N * N);
        HIP_CHECK(hipStreamSynchronize(st));
        pack_upper_tiles(c, h.data(), N);
    }
    DevBuf<double> dw;
    c->fp_T.ensure((size_t)3 * Tld);
    c->sw_scal.ensure(RES_STRIDE);
    c->sw_flags.ensure(4);
    c->sw_fring.ensure(4);
    ft_start(c, p, c->fp_T.p, 3, Tld, dw); // (TT's three parts)
    c->flow_armed_words = 0; // (no alpha of a sweep armed the hand-off slots of this launch)
    cge_fit_fused ff{};
    if (epi) { // (else no partial, no auc_part: nothing is wanted of the epilogue)
        ff = *epi;
        if (!(epi_want & 1)) ff.partial = nullptr;
        if (!(epi_want & 2)) ff.auc_part = nullptr;
    }
    ff.Lh = c->sw_Lh.p; ff.Ll = c->sw_Ll.p; ff.alpha = p.alpha;
    const cge_fit_fused *ff_dev = epi ? reinterpret_cast<const cge_fit_fused *>(c->sw_fused_epi.p) : nullptr; // (fused_upload's)
    FitForm fit;
    const int ran = ft_run(c, p, form, 0, eps, delta, fit, [&](AlphaSlot &sl) { // (a redo is form 0's: not packed, no epilogue)
        fit_undirected(c, N, dw.p, Tld, p.alpha, true, form == 2, form == 4 ? &ff : nullptr, form == 4 ? ff_dev : nullptr, fit, sl);
    });
    hook_down(c, p.T, c->fp_T.p + (i64)fit.tpar * Tld, N);
    HIP_CHECK(hipStreamSynchronize(st));
    if (form == 2) c->sw_PK.release(); // (held only while packed sweeps run)
    return ran;
}

static int ft_directed(cge_ctx *c, cge_fit_problem &p, int form, double eps, double delta) {
    hipStream_t st = c->stream;
    const i64 N = p.N;
    ft_matrices(c, p, false, true);
    if (form == 8) { // the upper tiles of GD
        std::vector<double> h((size_t)N * N);
        hook_down(c, h.data(), c->sw_GD.p, N * N);
        HIP_CHECK(hipStreamSynchronize(st));
        pack_upper_tiles(c, h.data(), N);
    }
    DevBuf<double> din, dout;
    c->sw_fring.ensure(4);
    c->sw_S1.ensure(N); c->sw_S2.ensure(N);
    c->sw_scal.ensure(RES_STRIDE);
    c->sw_flags.ensure(4);
    c->sw_fitstate.ensure(4);
    hook_up(c, c->sw_T1, p.T0, N);
    hook_up(c, c->sw_T2, p.T0b, N);
    hook_up(c, din, p.w, N);
    hook_up(c, dout, p.w2, N);
    HIP_CHECK(hipStreamSynchronize(st));
    ScoreGraph G;
    G.N = N;
    G.deg_in = din.p; G.deg_out = dout.p;
    FitForm fit;
    fit.dir_tiles = form == 7 ? 1 : form == 8 ? 2 : 0; // (else forms 0, 1, 3 only)
    const int ran = ft_run(c, p, form, 1, eps, delta, fit, [&](AlphaSlot &sl) { fit_directed(c, G, p.alpha, fit, sl); });
    hook_down(c, p.T, c->sw_T1.p, N);
    hook_down(c, p.Tb, c->sw_T2.p, N);
    HIP_CHECK(hipStreamSynchronize(st));
    if (form == 8) c->sw_PK.release(); // (held only while packed sweeps run)
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
    const i64 N = p.N, Tld = (i64)geo.Nt * 64;
    ft_matrices(c, p, true, false, true);
    m.Lh.swap(c->sw_Lh); m.Ll.swap(c->sw_Ll);
    c->pow_logs_N = c->pow_logs_blocked_N = 0; // (the context's logarithm left with the member)
    m.T.ensure((size_t)2 * Tld);
    ft_start(c, p, m.T.p, 2, Tld, m.w);
    return flow_problem_entry(m.Lh.p, m.Ll.p, p.alpha, epi, want, m.T.p, m.T.p + Tld, m.w.p, flags, N, Tld, geo);
}

// One launch shared by n members: its flags (four words per member, zeroed) and its scratch, the table -- `entry(i, flags)` stages
// member i and gives its entry --, the table's kernel through `launch(tab, flow)`, then every member's verdict and, through
// `down(p, entry)`, its iterates
template <class Tab, class Entry, class Launch, class Down>
static void ft_shared_launch(cge_ctx *c, cge_fit_problem *probs, int n, Entry entry, Launch launch, Down down) {
    DevBuf<int> flags;
    DevBuf<double> flow;
    flags.ensure((size_t)4 * n);
    HIP_CHECK(hipMemsetAsync(flags.p, 0, sizeof(int) * 4 * n, c->stream));
    Tab tab{};
    tab.n = n;
    for (int i = 0; i < n; i++) tab.p[i] = entry(i, flags.p + 4 * i);
    launch(tab, flow);
    for (int i = 0; i < n; i++) {
        probs[i].status = ft_verdict(c, tab.p[i].flags, &probs[i].iters) ? 0 : 1;
        down(probs[i], tab.p[i]);
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
// fit_flow_multi_kernel over n members (fit form 5, the fused chain)
template <class Entry>
static void ft_flow_multi(cge_ctx *c, cge_fit_problem *probs, int n, int NW, double eps, double delta, Entry entry) {
    ft_shared_launch<cge_flow_multi>(
        c, probs, n, entry, [&](cge_flow_multi &tab, DevBuf<double> &flow) { k_fit_flow_multi(c, tab, NW, eps, delta, flow); },
        [&](cge_fit_problem &p, const cge_flow_problem &q) { hook_down(c, p.T, q.Tout, p.N); });
}

// form 5: every problem with slots and flags of its own; nothing is wanted of the epilogue
static void ft_multi(cge_ctx *c, cge_fit_problem *probs, int n, const FlowGeometry *geo, double eps, double delta) {
    std::vector<FtMember> mem(n);
    ft_flow_multi(c, probs, n, geo[0].NW, eps, delta,
                  [&](int i, int *flags) { return ft_member(c, probs[i], geo[i], mem[i], flags, nullptr, 0); });
}

// form 6: every problem with its own power matrix, Tin / Tout, degrees and flags, as the directed members of a batch keep them
static void ft_dir_multi(cge_ctx *c, cge_fit_problem *probs, int n, const FlowGeometry *geo, double eps, double delta) {
    struct Member {
        DevBuf<double> GD, T, deg;
    };
    std::vector<Member> mem(n);
    ft_shared_launch<cge_flow_dir_multi>(
        c, probs, n,
        [&](int i, int *flags) {
            const cge_fit_problem &p = probs[i];
            const i64 N = p.N;
            Member &m = mem[i];
            ft_matrices(c, p, false, true);
            m.GD.swap(c->sw_GD); // (the context's power matrix leaves with the member)
            hook_up2(c, m.T, p.T0, N, p.T0b, N);
            hook_up2(c, m.deg, p.w, N, p.w2, N);
            HIP_CHECK(hipStreamSynchronize(c->stream));
            cge_flow_dir_problem q{};
            q.GD = m.GD.p;
            q.Tin = m.T.p; q.Tout = m.T.p + N;
            q.deg_in = m.deg.p; q.deg_out = m.deg.p + N;
            q.flags = flags;
            q.N = N; q.Tld = (i64)geo[i].Nt * 64; q.Nt = geo[i].Nt; q.G = geo[i].G;
            return q;
        },
        [&](cge_flow_dir_multi &tab, DevBuf<double> &flow) { k_fit_flow_dir_multi(c, tab, geo[0].NW, eps, 1.0, delta, flow); },
        [&](cge_fit_problem &p, const cge_flow_dir_problem &q) {
            hook_down(c, p.T, q.Tin, p.N);
            hook_down(c, p.Tb, q.Tout, p.N);
        });
}

void host_fit_test(cge_ctx *c, cge_fit_problem *probs, int n, int directed, int form, double eps, double delta, int *form_ran) {
    if (!directed && form == 6) CGE_THROW(CGE_E_ARG, "fit_test: form 6 is directed only");
    if (!directed && (form == 7 || form == 8)) CGE_THROW(CGE_E_ARG, "fit_test: form %d is directed only", form);
    if (n > 1 && form != 5 && form != 6) CGE_THROW(CGE_E_ARG, "fit_test: %d problems in one call are form 5 only", n);
    if (n > CGE_BATCH_MAX) CGE_THROW(CGE_E_ARG, "fit_test: form %d takes at most %d problems", form, CGE_BATCH_MAX);
    if (directed && (form == 2 || form == 4 || form == 5)) CGE_THROW(CGE_E_ARG, "fit_test: form %d is undirected only", form);
    if ((form == 4 || form == 5) && !c->opt_pow_exp2)
        CGE_THROW(CGE_E_ARG, "fit_test: form %d makes its power matrix from the stored logarithm (option pow_exp2)", form);
    if (!(eps > 0.0) || !(delta >= 0.0)) CGE_THROW(CGE_E_ARG, "fit_test: eps > 0 and delta >= 0");
    const bool multi = form == 5 || form == 6;
    FlowGeometry geo[CGE_BATCH_MAX];
    int sumG = 0;
    const int cus = device_cus(c);
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

// ---- the testing hook of the fused chain (include/cge_hip_testing.h: cge_fused_chain_test) -----------------------------------
// One alpha as enqueue_alpha / host_batch_sweep run it on the fused path, on a caller's problem: the layout and its tables, the
// epilogue's table, the fit with its epilogue's outputs wanted, the bins and the divergence.  A problem is prepared on the
// context's buffers, as a sweep prepares it; the problems of a shared launch then take them along (FcMember), as hand_off does.
namespace {
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
    const std::vector<i32> hcomm = hook_comm0("fused_chain_test", p.comm, N, C);
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
    std::vector<i32> old2new(N), comm_new(N);
    for (i64 q = 0; q < N; q++) {
        old2new[m.order[q]] = (i32)q;
        comm_new[q] = hcomm[m.order[q]];
    }
    m.D = hook_permuted(m.order, p.D, true); m.w = hook_permuted(m.order, p.w, false); m.T0 = hook_permuted(m.order, p.T0, false);
    m.T.assign(N, std::nan(""));
    hook_up(c, m.comm, comm_new.data(), N);
    hook_layout_tables(c, lay, N, C, 0);
    fill_nan(c, c->sw_bt_part.p, sizeof(double) * lay.bt_total);
    hook_down(c, p.fc, c->sw_bt_fc.p, Nt);
    hook_down(c, p.ns, c->sw_bt_ns.p, Nt);
    hook_down(c, p.base, c->sw_bt_base.p, Nt * Nt);
    // the tally's operands: the caller's, T's indices through old2new
    if (S > 0) {
        std::vector<i32> ax((size_t)4 * S);
        for (i64 k = 0; k < 4 * S; k++) ax[k] = old2new[p.aidx[k]];
        hook_up(c, m.aidx, ax.data(), 4 * S);
        hook_up2(c, m.afac, p.afac, 8 * S, p.aden, (i64)CGE_PARTIAL_BLOCKS); // (the blocks' weight sums behind the factors, as fused_tables keeps them)
        hook_up(c, m.dpos, p.dpos, S);
        hook_up(c, m.dneg, p.dneg, S);
        hook_up(c, m.wts, p.wts, S);
        m.apw.ensure((size_t)2 * S);
        fill_nan(c, m.apw.p, sizeof(double) * 2 * S);
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
        hook_up(c, m.epi_dev, reinterpret_cast<const char *>(&m.epi), (i64)sizeof(cge_fit_fused));
    } else
        fused_upload(c, std::vector<cge_fit_fused>(1, m.epi));
    fill_nan(c, m.epi.auc_part, sizeof(double) * 2 * CGE_PARTIAL_BLOCKS); // (until the epilogue writes)
    // vect_B with its guard of NaNs behind it, and vect_C (zeros where the caller has none)
    std::vector<double> hv((size_t)(m.vlen + CGE_VECT_B_GUARD), std::nan("")), hc((size_t)m.vlen, 0.0);
    if (p.vC) std::memcpy(hc.data(), p.vC, sizeof(double) * m.vlen);
    hook_up(c, m.vB, hv.data(), (i64)hv.size());
    hook_up(c, m.vC, hc.data(), m.vlen);
    m.fpart.ensure((size_t)2 * CGE_PARTIAL_BLOCKS);
    HIP_CHECK(hipStreamSynchronize(st)); // (the host copies go out of scope)
}

// the fit of a prepared member, as the fit's hook takes a problem: in the sweep's numbering, the iterate into m.T
static cge_fit_problem fit_problem_of(FcMember &m, const cge_fused_chain_problem &p) {
    cge_fit_problem fp{};
    fp.D = m.D.data(); fp.w = m.w.data(); fp.T0 = m.T0.data(); fp.T = m.T.data(); fp.N = p.N; fp.alpha = p.alpha;
    return fp;
}

// what a problem's launch left: the fit's verdict, the iterate in the caller's numbering, the tile partials (before the bins), the
// tallies, the powers
static void fc_collect(cge_ctx *c, cge_fused_chain_problem &p, FcMember &m, const cge_fit_problem &fp, const double *partial) {
    const i64 S = (p.want & 2) ? p.S : 0;
    p.iters = fp.iters;
    p.status = fp.status;
    for (i64 q = 0; q < p.N; q++) p.T[m.order[q]] = m.T[q];
    if (p.order) std::memcpy(p.order, m.order.data(), sizeof(i32) * p.N);
    p.bt_total = m.bt_total;
    hook_down(c, p.partials, partial, m.bt_total);
    hook_down(c, p.part, m.epi.auc_part, 2 * CGE_PARTIAL_BLOCKS);
    if (S > 0) hook_down(c, p.apw, m.apw.p, 2 * S);
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
    const int cus = device_cus(c);
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
    HookOptions restore{c};
    c->opt_fit_fused = 1; c->opt_exact_relabel = true; c->opt_test_bvec_plain = 0;
    if (c->opt_fit_persistent == 1) c->opt_fit_persistent = 0;
    std::vector<FcMember> mem(n);
    if (n == 1) { // ---- fit_flow_kernel<.., true>, as enqueue_alpha launches it, then bins_js_kernel -------------------------------
        cge_fused_chain_problem &p = probs[0];
        FcMember &m = mem[0];
        fc_prepare(c, p, m, false);
        cge_fit_problem fp = fit_problem_of(m, p);
        ft_undirected(c, fp, 4, eps, delta, &m.epi, p.want);
        fc_collect(c, p, m, fp, c->sw_bt_part.p);
        if ((p.want & 1) && p.status == 0) k_bins_js(c, c->sw_cm_off.p, p.N, p.C, m.vC.p, m.vB.p, p.n_modes, m.fpart.p);
    } else { // ---- fit_flow_multi_kernel over the members, then the batch's bins / JS launches ------------------------------------------
        std::vector<cge_fit_problem> fps(n);
        ft_flow_multi(c, fps.data(), n, geo[0].NW, eps, delta, [&](int i, int *flags) {
            FcMember &m = mem[i];
            fc_prepare(c, probs[i], m, true);
            fps[i] = fit_problem_of(m, probs[i]);
            return ft_member(c, fps[i], geo[i], m.fit, flags, reinterpret_cast<const cge_fit_fused *>(m.epi_dev.p), probs[i].want);
        });
        cge_bins_multi bins{};
        cge_js_multi js{};
        int nb = 0, nj = 0;
        i64 maxC = 0;
        for (int i = 0; i < n; i++) {
            cge_fused_chain_problem &p = probs[i];
            FcMember &m = mem[i];
            fc_collect(c, p, m, fps[i], m.part.p);
            if (!((p.want & 1) && p.status == 0)) continue;
            bins.p[nb++] = cge_bins_problem{m.part.p, m.cm_off.p, m.fc.p, m.ns.p, m.base.p, p.C, geo[i].Nt, 0, m.vB.p};
            maxC = std::max(maxC, p.C);
            m.jspart.ensure((size_t)2 * 3 * CGE_PARTIAL_BLOCKS);
            hook_js_entries(js, nj, m.vC.p, m.vB.p, m.vlen, p.C, p.n_modes, m.jspart.p, m.fpart.p);
        }
        k_bins_js_multi(c, bins, nb, maxC, js, nj);
    }
    for (int i = 0; i < n; i++) {
        cge_fused_chain_problem &p = probs[i];
        FcMember &m = mem[i];
        std::vector<double> hf((size_t)2 * CGE_PARTIAL_BLOCKS, std::nan(""));
        const bool binned = (p.want & 1) && p.status == 0;
        if (binned) hook_down(c, hf.data(), m.fpart.p, 2 * CGE_PARTIAL_BLOCKS);
        hook_down(c, p.vectB, m.vB.p, m.vlen + CGE_VECT_B_GUARD);
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
    const i64 S = io->S, n = c->n, N = io->N;
    const i64 m = c->edges_sharded ? c->m_total : c->m; // (a sharded list: pos / pos_in are rows of the caller's whole list)
    const int directed = io->directed != 0, form = io->form;
    const bool landmark_form = form == 1 || form == 4, exact_form = form == 2 || form == 3 || form == 5;
    // the stages that run
    const bool draw = io->draw_route != 0;
    const bool pairs_in = io->pi_in || io->pj_in || io->ni_in || io->nj_in || io->wts_in;
    const bool draws_in = io->pos_in || io->neg_i_in || io->neg_j_in;
    const bool dist = io->dpos || io->dneg || (landmark_form && !io->dpos_in);
    const bool prep = io->pi || io->pj || io->ni || io->nj || io->wts || ((dist || form != 0) && !pairs_in);
    // ---- the checks --------------------------------------------------------------------------------------------------------------
    if (S < 1 || S >= ((i64)1 << 28)) CGE_THROW(CGE_E_ARG, "local_score_test: S = %lld samples", (long long)S);
    if ((c->rows_sharded || c->edges_sharded) && !io->sharded)
        CGE_THROW(CGE_E_ARG, "local_score_test: not with option shard_rows / shard_ingest (every row and edge on one rank), unless sharded = 1");
    if ((c->rows_sharded || c->edges_sharded) && form != 0) // (sharded = 1: Draw, Prepare and Distances run collectively)
        CGE_THROW(CGE_E_ARG, "local_score_test: the tally forms are refused under option shard_rows / shard_ingest (form = %d)", form);
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
    if (dist && (!c->Xr.p || c->d <= 0 || c->Xr.n < (size_t)(lm_rows(c) * c->d)))
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
        if (!flow_fused_applies(c, N))
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
        hook_down(c, io->pos, d_pos.p, S);
        hook_down(c, io->neg_i, d_ni.p, S);
        hook_down(c, io->neg_j, d_nj.p, S);
        hook_down(c, io->attempt, c->samp_attempt.p, S);
    }
    // ---- Prepare -----------------------------------------------------------------------------------------------------------------
    if (prep) {
        if (draws_in) {
            hook_up(c, d_pos, io->pos_in, S);
            hook_up(c, d_ni, io->neg_i_in, S);
            hook_up(c, d_nj, io->neg_j_in, S);
        }
        if (io->pos2_in) hook_up(c, d_pos2, io->pos2_in, S);
        ds.pi.ensure(S); ds.pj.ensure(S); ds.ni.ensure(S); ds.nj.ensure(S); ds.wts.ensure(S);
        k_prep_samples(c, d_pos.p, io->pos2_in ? d_pos2.p : d_pos.p, d_ni.p, d_nj.p, c->src.p, c->dst.p, c->w.p, S, directed, ds.pi.p,
                       ds.pj.p, ds.ni.p, ds.nj.p, ds.wts.p);
        hook_down(c, io->pi, ds.pi.p, S);
        hook_down(c, io->pj, ds.pj.p, S);
        hook_down(c, io->ni, ds.ni.p, S);
        hook_down(c, io->nj, ds.nj.p, S);
        hook_down(c, io->wts, ds.wts.p, S);
    } else if (pairs_in) {
        hook_up(c, ds.pi, io->pi_in, S);
        hook_up(c, ds.pj, io->pj_in, S);
        hook_up(c, ds.ni, io->ni_in, S);
        hook_up(c, ds.nj, io->nj_in, S);
        hook_up(c, ds.wts, io->wts_in, S);
    }
    // ---- Distances ---------------------------------------------------------------------------------------------------------------
    if (dist) {
        ds.dpos.ensure(S); ds.dneg.ensure(S);
        sampled_pair_dist(c, c->Xr.p, c->d, ds.pi.p, ds.pj.p, S, io->hi, ds.dpos.p);
        sampled_pair_dist(c, c->Xr.p, c->d, ds.ni.p, ds.nj.p, S, io->hi, ds.dneg.p);
        hook_down(c, io->dpos, ds.dpos.p, S);
        hook_down(c, io->dneg, ds.dneg.p, S);
    }
    if (io->dpos_in) { // (behind the copies out of the distance stage, when that ran for its outputs)
        hook_up(c, ds.dpos, io->dpos_in, S);
        hook_up(c, ds.dneg, io->dneg_in, S);
    }
    // ---- Tally -------------------------------------------------------------------------------------------------------------------
    DevBuf<double> dTa, dTb, dvw, dlw, dout2;
    DevBuf<i32> dv2l, do2n;
    std::vector<double> hpart(2 * CGE_PARTIAL_BLOCKS, std::nan(""));
    if (landmark_form) {
        hook_up(c, dv2l, io->v2l, n);
        hook_up(c, dvw, io->vw, n);
        hook_up(c, dlw, io->lweight, N);
        if (io->old2new) hook_up(c, do2n, io->old2new, N);
    }
    const bool plain_tally = (form >= 1 && form <= 3) || form == 5;
    if (plain_tally) {
        hook_up(c, dTa, io->Ta, N);
        if (io->Tb) hook_up(c, dTb, io->Tb, N);
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
        const bool packed = form == 3 || form == 5; // (5: ordered pairs, either side of the diagonal -- the directed sweep's)
        if (packed) pack_upper_tiles(c, io->GD, N); // the upper tiles of GD
        else hook_up(c, c->sw_GD, io->GD, N * N);
        k_auc_exact(c, packed ? c->sw_PK.p : c->sw_GD.p, dTa.p, io->Tb ? dTb.p : dTa.p, N, ds.pi.p, ds.pj.p, ds.ni.p, ds.nj.p, ds.wts.p, S,
                    dout2.p, nullptr, packed);
    }
    if (plain_tally) {
        hook_down(c, hpart.data(), c->auc_part.p, 2 * CGE_PARTIAL_BLOCKS);
        hook_down(c, io->out2, dout2.p, 2);
    }
    if (form == 4) {
        c->sw_scal.ensure(RES_STRIDE);
        fill_nan(c, c->sw_scal.p + RES_AUC, sizeof(double) * 2 * CGE_PARTIAL_BLOCKS); // (until the epilogue writes)
        OrigView orig;
        orig.n = n; orig.v2l = dv2l.p; orig.vw = dvw.p; orig.lweight = dlw.p;
        ScoreGraph G;
        G.N = N;
        std::vector<cge_fit_fused> h_epi;
        fused_tables(c, G, &orig, io->old2new ? do2n.p : nullptr, 1, 0, S, true, h_epi);
        std::vector<double> hT(N);
        cge_fit_problem p{};
        p.D = io->D; p.w = io->w; p.T0 = io->T0; p.T = io->T ? io->T : hT.data(); p.N = N; p.alpha = io->alpha;
        ft_undirected(c, p, 4, io->eps, io->delta, &h_epi[0]);
        io->iters = p.iters;
        io->status = p.status;
        hook_down(c, hpart.data(), c->sw_scal.p + RES_AUC, 2 * CGE_PARTIAL_BLOCKS);
        hook_down(c, io->aidx, ds.aidx.p, 4 * S);
        hook_down(c, io->afac, ds.afac.p, 8 * S);
        hook_down(c, io->aden, ds.afac.p + 8 * S, (i64)CGE_PARTIAL_BLOCKS);
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (form == 3 || form == 5) c->sw_PK.release(); // (held only while packed sweeps run)
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
    const std::vector<i32> hcomm = hook_comm0("sweep_setup_test", io->comm, N, C);
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
    hook_up(c, c->s_emb, io->emb, N * d);
    hook_up(c, c->s_dist, io->dist, N);
    hook_up(c, c->s_comm, hcomm.data(), N);
    ScoreGraph G;
    G.N = N; G.d = d; G.C = C;
    G.emb = c->s_emb.p; G.dist = c->s_dist.p; G.comm = c->s_comm.p;
    if (io->vw) {
        hook_up(c, c->s_vw, io->vw, N);
        G.vw = c->s_vw.p;
    }
    // ---- the degrees (score_host.cpp: edge_degrees) ----------------------------------------------------------------------------
    DevBuf<i32> e_src, e_dst;
    DevBuf<double> e_w;
    if (edges) {
        hook_up(c, e_src, io->src, m);
        hook_up(c, e_dst, io->dst, m);
        if (io->w) hook_up(c, e_w, io->w, m);
        edge_degrees(c, e_src.p, e_dst.p, io->w ? e_w.p : nullptr, m, N, c->s_star);
        G.deg_in = c->s_degin.p;
        G.deg_out = c->s_degout.p;
        hook_down(c, io->deg_out, c->s_degout.p, N);
        hook_down(c, io->deg_in, c->s_degin.p, N);
        hook_down(c, io->star, c->s_star.p, N);
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
        hook_down(c, io->order, c->sw_rl_order.p, N);
        hook_down(c, io->old2new, lay.old2new.p, N);
    }
    hook_down(c, io->emb_rl, G.emb, N * d);
    hook_down(c, io->comm_rl, G.comm, N);
    if (io->vec_rl) {
        const double *vec[4] = {G.dist, G.vw, G.deg_in, G.deg_out};
        for (int q = 0; q < 4; q++)
            if (vec[q]) hook_down(c, io->vec_rl + q * N, vec[q], N);
    }
    // ---- D, its extrema and normalisation, the community tables, the start vectors ------------------------------------------
    if (io->D_raw || want_prep) { c->sw_D.ensure((size_t)N * N); c->sw_GD.ensure((size_t)N * N); }
    if (io->D_raw) {
        k_dist_matrix(c, G.emb, G.dist, N, d, c->sw_D.p);
        hook_down(c, io->D_raw, c->sw_D.p, N * N);
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (!want_prep) return;
    io->Tld = prepare_distances(c, G, lay, directed, false);
    hook_down(c, io->lo_hi, c->sw_lohi.p, 2);
    hook_down(c, io->D, c->sw_D.p, N * N);
    hook_down(c, io->cm_off, c->sw_cm_off.p, C + 1);
    hook_down(c, io->cm_mem, c->sw_cm_mem.p, N);
    hook_down(c, io->cm_pos, c->sw_cm_pos.p, N);
    hook_down(c, io->T1, c->sw_T1.p, N);
    hook_down(c, io->T2, c->sw_T2.p, N);
    hook_down(c, io->TT, c->fp_T.p, 3 * io->Tld);
    HIP_CHECK(hipStreamSynchronize(st));
    if (!want_log && !want_gd) return;
    // ---- the logarithm, and the power of one alpha from it ------------------------------------------------------------------
    const bool upper = form == 0 ? landmarks && !directed : form >= 2, blocked = form == 0 ? lay.fuse : form == 3;
    const i64 len = blocked ? blocked_len : N * N;
    if (c->opt_pow_exp2) { // (a NaN in both; k_pow_prepare's own ensure finds them large enough)
        c->sw_Lh.ensure((size_t)len); c->sw_Ll.ensure((size_t)len);
        fill_nan(c, c->sw_Lh.p, sizeof(double) * len);
        fill_nan(c, c->sw_Ll.p, sizeof(float) * len);
    }
    k_pow_prepare(c, c->sw_D.p, N, upper, blocked);
    io->log_form_ran = c->pow_logs_blocked_N == N ? 3 : c->pow_logs_N != N ? 0 : c->pow_logs_upper ? 2 : 1;
    io->log_count = io->log_form_ran == 0 ? 0 : len;
    if (want_log && io->log_form_ran != 0) {
        hook_down(c, io->Lh, c->sw_Lh.p, len);
        hook_down(c, io->Ll, c->sw_Ll.p, len);
    }
    if (want_gd && io->log_form_ran != 3) {
        fill_nan(c, c->sw_GD.p, sizeof(double) * N * N); // (as ft_matrices does)
        k_pow_matrix(c, c->sw_D.p, N, io->alpha, c->sw_GD.p, upper);
        hook_down(c, io->GD, c->sw_GD.p, N * N);
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
    dlohi.ensure(2); PK.ensure((size_t)NT * CGE_TILE_DOUBLES);
    hook_up(c, demb, emb, N * d);
    hook_up(c, ddiag, diag, N);
    k_packed_extrema(c, demb.p, ddiag.p, N, d, dlohi.p);
    k_packed_gd(c, demb.p, ddiag.p, N, d, dlohi.p, alpha, pow_method, PK.p);
    std::vector<double> h((size_t)NT * CGE_TILE_DOUBLES);
    hook_down(c, h.data(), PK.p, (i64)h.size());
    hook_down(c, lo_hi, dlohi.p, 2);
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
