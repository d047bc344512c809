// sweep_internal.hpp -- what the kernel-level testing hooks (sweep_hooks.cpp) take from the alpha sweep (wgcl_host.cpp), and
// nothing else: the functions a hook may call are the ones declared here.  Included by those two files only; every function is
// defined, and described, in wgcl_host.cpp.
#pragma once
#include "common.hpp"

// How a sweep lays its score graph out: the community -> members CSR, whether the graph is relabelled by community (the sweep's
// numbering) and whether the rest of an alpha's chain rides on the fit's launch (vect_B by tiles or not: c->bvec_blocks).
struct SweepLayout {
    std::vector<i32> cm_off, cm_mem; // community -> members, in the sweep's numbering
    bool relabel = false, fuse = false;
    i64 bt_total = 0;    // tile partials in all
    DevBuf<i32> old2new; // (relabel) a vertex's number in the sweep
};

// What the host keeps of an alpha in flight until it collects it (two at most: slot = alpha index mod 2)
struct AlphaSlot {
    bool fit_async = false;      // the fit was only enqueued: its verdict arrives with the alpha's scalars
    bool fused = false;          // the rest of the chain rode on the fit's launch
    bool shared_verdict = false; // N > 1, tallies split: the verdict of the fit travelled with the all-reduced tallies
    int t0_par = 0;              // the part of TT that held T_0 of this alpha
    i64 iters = 0;
    const double *Ta = nullptr, *Tb = nullptr; // where this alpha's iterate lives (directed: Tout, Tin) until the next alphas overwrite it
};

// The form of the fit from alpha to alpha (a persistent form, once given up, stays given up for the sweep), the part of TT that
// holds the current iterate (undirected) and the last iteration count (the first batch of a launch-per-iteration fit).  eps,
// delta: the step and the stopping threshold -- a sweep's are the reference's (0.25 undirected :119, 0.9 directed :434; delta
// :35); the testing hook cge_fit_test passes its caller's.
struct FitForm {
    bool persistent = false, persistent_dir = false;
    int dir_tiles = 0; // a directed launch-per-iteration fit by the tile pair: 1 on the row-major GD, 2 on the packed tiles (sw_PK)
    int tpar = 0;
    i64 prev_iters = 16;
    double eps = 0.25, delta = AlphaBook::delta;
};

// ---- the set-up of a sweep
void sampled_pair_dist(cge_ctx *c, const double *Xr, i64 d, const i32 *pi, const i32 *pj, i64 S, double den, double *out);
void layout_tables(cge_ctx *c, const i32 *hcomm, i64 N, i64 C, int directed, bool landmarks, bool force_relabel, SweepLayout &lay,
                   bool packed_req = false);
void plan_layout(cge_ctx *c, ScoreGraph &G, const OrigView *orig, int directed, SweepLayout &lay, bool packed_req,
                 bool force_relabel = false);
void community_tables(cge_ctx *c, const SweepLayout &lay, i64 N, i64 C, WordPacker &pk, std::vector<i32> &cm_pos);
i64 prepare_distances(cge_ctx *c, const ScoreGraph &G, const SweepLayout &lay, int directed, bool packed);
cge_fit_fused fused_entry(cge_ctx *c, const i32 *comm, i64 S, const double *dpos, const double *dneg, const double *wts);
void fused_upload(cge_ctx *c, const std::vector<cge_fit_fused> &h_epi);
void fused_tables(cge_ctx *c, const ScoreGraph &G, const OrigView *orig, const i32 *old2new, i64 n_sets, i64 s0, i64 s1,
                  bool fuse_auc, std::vector<cge_fit_fused> &h_epi);
// ---- one alpha's fit
bool persistent_wanted(const cge_ctx *c, i64 N);
void fit_undirected(cge_ctx *c, i64 N, const double *w, i64 Tld, double alpha, bool upper, bool packed, const cge_fit_fused *ff,
                    const cge_fit_fused *ff_dev, FitForm &fit, AlphaSlot &sl);
void fit_directed(cge_ctx *c, const ScoreGraph &G, double alpha, FitForm &fit, AlphaSlot &sl);
void leave_persistent(cge_ctx *c, int directed, FitForm &fit, const AlphaSlot &sl);
