/* cge_hip_testing.h -- host-only hooks of libcge_hip.so used by the CPU test-suite (no GPU needed).
 * They expose the product's own host routines (NOT the oracle's) so that `-m "not gpu"` tests can
 * check them against the oracle. */
#ifndef CGE_HIP_TESTING_H
#define CGE_HIP_TESTING_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* principal eigenvector of a symmetric d x d matrix (replaces eigvecs(A)[:, end], src/landmarks.jl:99) */
int cge_host_eig_top(const double *A, int64_t d, double *v);
/* cge_score_batch's launch groups for members of N[k] landmarks on `cus` CUs (no device work): group_of[k] = the launch group of
 * member k, -1 for a member outside the fused fit's geometry (scored on its own); returns the number of groups.  Members keep
 * their order; a group closes when the next member's workgroups would exceed `cus`, its waves per workgroup differ, or it holds
 * 16 members. */
int cge_batch_pack_test(const int64_t *N, int64_t K, int cus, int32_t *group_of);
/* host-only (no device work, no context): the one geometry of the persistent fits (flow_geometry), undirected and directed, for N
 * vertices on `cus` CUs, as every single launch and every member of a shared launch takes it.  *applies = 0: the form declines
 * (the other outputs are not written).  Else G workgroups of NW waves (4 or 8), and NSB = 1 or 2 quarter blocks per workgroup. */
int cge_fit_dir_geometry_test(int64_t N, int cus, int *applies, int *G, int *NW, int *NSB);
/* host-only: the one layout of a problem's hand-off slots (flow_slots) for N vertices (1 .. 4096) and Tld = 64 ceil(N / 64), in
 * doubles from the start of the problem's region: out = the offsets of the sync words, the T ring, f and P, and the region's
 * length.  Problems of a shared launch lie back to back, each at the sum of the lengths before it. */
int cge_fit_slots_test(int64_t N, int directed, int64_t out[5]);
/* cge_batch_pack_test for the members of a directed batch: a member of N[k] landmarks shares the fit's launch when N[k] >= 256,
 * the directed geometry applies with NSB = 1 and G <= cus / 2 (else group_of[k] = -1); the groups close by the same rule. */
int cge_batch_pack_dir_test(const int64_t *N, int64_t K, int cus, int32_t *group_of);
/* the sampler's counter-based draw of positive rows: pos_idx[k] in 1..m (no device work) */
int cge_host_pos_draw(int64_t seed, int64_t stream_id, int64_t S, int64_t m, int64_t *pos_idx);
/* kernel-level hook (needs the GPU): principal eigenvectors of T symmetric d x d matrices (row-major, back to
 * back) by the batched device solvers that landmarks uses (d <= 128: register-resident; d <= 512: global-memory
 * resident); returns CGE_E_ARG for d > 512 */
int cge_group_eig(void *ctx, const double *A, int64_t T, int64_t d, double *v);
/* kernel-level hook (needs the GPU): the statistics stage of a landmark split and the side sums for T caller-supplied groups of
 * the resident embedding and vertex weights, by the split's own batch builder, chunk tables and launch wrappers (the member
 * lists and the means are placed in the arenas a runsplit keeps them in; the arenas start from zero, as for a runsplit).
 *   ids: the groups' 0-based row ids back to back, group t = ids[task_row_off[t] .. task_row_off[t + 1]); the groups are
 *   disjoint, at least one row each, ids in any order (R = task_row_off[T] rows in all).
 *   Out: mean[T][d]; sw[T] = the groups' weight sums (written only when the means are computed); cov[T][d][d] =
 *   sum_j w_j (x_j - mean)(x_j - mean)^T; vec[T][d] = its principal eigenvector; z[R] = the rows' projections
 *   sum_c (x_jc - mean_c) sqrt(w_j) vec_c.
 *   mean_in (optional, T x d): every group's mean is known -- it is gathered from the means arena (k_gather_means) and not
 *   computed (k_group_mean), as for a child that inherits its mean from its parent's side sums; mean returns it unchanged.
 *   side (optional, R flags 0 / 1 / 2; d <= 512) with sums[T][2][2 d + 1]: per group and side 1, 2 the sums of w x^2 [d],
 *   w x [d] and w over the rows with that flag (0: in neither).
 * CGE_E_ARG with a message for an empty group, an id outside the resident rows or in two groups, a flag above 2 or a context with
 * option shard_rows. */
int cge_group_stats_test(void *ctx, const int32_t *ids, const int32_t *task_row_off, int64_t T, const uint8_t *side, const double *mean_in,
                         double *mean, double *sw, double *cov, double *vec, double *z, double *sums);
/* kernel-level hook (needs the GPU): the cut stage of a landmark split -- the per-group sort of the projections, the rule's
 * one-dimensional cut, the children's member lists, values and means -- for T caller-supplied groups (as for
 * cge_group_stats_test, here of at least 3 rows each: shorter groups never reach the device) by the split's own batch builder,
 * launch wrappers and collect step, the generic host path of the rss tasks the sorted form declines included.  The arenas start
 * from zero and the counter of tie tasks is zeroed first.
 *   method: a CGE_METHOD_* code.  z (R doubles, one per row in ids order): the projections, in place of the statistics stage, so
 *   a caller decides every tie and every order; z == NULL: the statistics stage runs first (the whole split).  force_generic
 *   (rss only): non-zero sends every task through the generic host path instead of the sorted form.
 *   Out: rc[T] = the task's code (CGE_OK, CGE_E_HOMOGENEOUS, CGE_E_EMPTY_CLUSTER); nlow[T] = rows of the low child;
 *   children[R] = the children lists, task t at task_row_off[t], low child first; vlow[T], vhigh[T] = the children's values as
 *   the split books them (DBL_EPSILON for a one-row child; 0 for a failed task); cmeans[T][2][d] = the children's means from the
 *   means arena (NaN for a failed task); route[T] = 0 the device form, 1 the generic host path; *ties = tasks of the size /
 *   diameter rules that held a row ON the cut.
 * CGE_E_ARG with a message, before any launch, for a group of fewer than 3 rows, an id outside the resident rows or in two
 * groups, an unknown method, rss / rss2 with d > 512 or a context with option shard_rows (size / diameter with d > 512: the
 * side sums behind the cut refuse, CGE_E_ARG too). */
int cge_group_cut_test(void *ctx, const int32_t *ids, const int32_t *task_row_off, int64_t T, int method, const double *z, int force_generic,
                       int32_t *rc, int32_t *nlow, int32_t *children, double *vlow, double *vhigh, double *cmeans, int32_t *route,
                       int32_t *ties);
/* kernel-level hook (needs the GPU): the bound matrix of the pruned diameter for the resident embedding and a caller-supplied
 * landmark assignment -- the layout, the reference points, the gather with its fitness verdict and ONE bound pass, by the launch
 * wrappers cge_score's diameter uses.  v2l[i] in 1..N (every landmark non-empty; its centroid is the mean of its members),
 * lcomm[a] in 1..C (every community non-empty).  pass: 0 fp64, 1 f32, 2 the bf16 split (CGE_E_ARG for d > 128, where it does
 * not apply).  P (N x nref doubles, row-major): P[a][r] >= max over the members i of a of ||x_i - ref_r||^2 on the centred rows;
 * nref = C reference points (the community centroids) for C >= 32, else the N landmark centroids; pass_ran = the pass after
 * the fitness verdict (0 when a centred value is unfit for the low-precision passes).  Optional: ref_points (nref x d,
 * row-major, uncentred) and mean (d): what the device centred with */
int cge_diameter_bounds_test(void *ctx, const int64_t *v2l, int64_t N, const int64_t *lcomm, int64_t C, int pass, double *P,
                             int64_t *nref, int *pass_ran, double *ref_points, double *mean);
/* kernel-level hook (needs the GPU): the mutual squared distances of caller-supplied reference points as the pruned diameter
 * forms them for its candidate selection -- refs (nref x d doubles, row-major, d of the resident embedding) are centred with the
 * resident embedding's mean into the feature-major copy (the gather of the bound pass's reference operand), then one launch of
 * the distance kernel.  rd2 (nref x nref, row-major): rd2[a][b] = the sequential sum over k ascending of fl(fl(a_k - m_k) -
 * fl(b_k - m_k))^2, unfused.  Optional: mean (d), what the device centred with */
int cge_ref_dist2_test(void *ctx, const double *refs, int64_t nref, double *rd2, double *mean);
/* kernel-level hook (needs the GPU): the stage of a landmark run that turns an assignment into the landmark graph, on a caller's
 * v2l[n] (ids in 1..N) over the resident graph and vertex data, by the stage's own functions and launch wrappers (the ones
 * cge_landmarks_run and cge_score call).  Every output pointer may be NULL: that work is skipped.  The call drops the results of
 * an earlier cge_landmarks_run (its buffers are used).
 *   Aggregate (src/landmarks.jl:387-430; needs the embedding and the vertex data, every landmark with at least one member): the
 *   landmark -> members index with ascending members, then k_landmark_aggregate: lemb[N][d] (row-major), lweight[N], dii[N],
 *   lcomm[N] (0-based community of the last member).
 *   The landmark-pair matrix (:433-451; landmarks without a member allowed): wedges[N][N] row-major and *positive, the count of
 *   its positive entries (on and above the diagonal when undirected), from the share `part` of `nparts` of the edges that a rank
 *   takes -- of the chunks of the blocked edge list for the tiled form, of the m edges for the gather form.
 *   wedge_form 0: what a run picks; 1: the tiled two-pass form (k_wedge_scatter_blocked); 2: k_edge_scatter + k_compact_count.
 *   Degrees of the directed score from that matrix: deg_out[N], deg_in[N], star[N] by k_wedge_degrees; deg_block[world][3 N] by
 *   k_wedge_degrees_block on the row block of each of `world` pretend ranks; u_deg_out, u_deg_in, u_star [N] = k_degrees_unpack
 *   of the blocks' sum (added in rank order).
 *   Out: form_ran (1 or 2), n_chunks (of the blocked edge list; 0 when there is none), and the tiled form's geometry for this
 *   share when it ran (rshift, colbits, ntile; -1 otherwise).
 * CGE_E_ARG with a message, before any launch: an id outside 1..N, missing residents, a landmark without a member when the
 * aggregate is asked for, part / nparts / world out of range, a context with option shard_rows or shard_ingest, wedge_form 1 where
 * the blocked edge list or the geometry declines. */
typedef struct cge_landmark_graph_io {
    const int64_t *v2l;
    int64_t N;
    int32_t directed, wedge_form;
    int64_t part, nparts, world;
    double *lemb, *lweight, *dii;
    int32_t *lcomm;
    double *wedges;
    int64_t *positive;
    double *deg_out, *deg_in;
    int32_t *star;
    double *deg_block, *u_deg_out, *u_deg_in;
    int32_t *u_star;
    int64_t n_chunks, ntile;
    int32_t form_ran, rshift, colbits, pad;
} cge_landmark_graph_io;
int cge_landmark_graph_test(void *ctx, cge_landmark_graph_io *io);
/* host-only (no device work, no context): the geometry of the tiled form of the landmark-pair matrix for N landmarks over
 * n_chunks chunks of a unit (weighted = 0) or weighted edge list, as the launch reads it.  *applies = 0: the form declines (the
 * other outputs are not written).  Else tiles of 1 << rshift rows, 16-bit keys of rshift + colbits bits, ntile tiles and the
 * dynamic LDS in bytes of pass 1 (wedge_pass_kernel) and pass 2 (wedge_tile_kernel). */
int cge_wedge_geometry_test(int64_t N, int weighted, int64_t n_chunks, int *applies, int *rshift, int *colbits, int64_t *ntile,
                            int64_t *lds_pass1, int64_t *lds_pass2);
/* out[i] = (1 - x[i])^alpha on the device (host vectors): method 0 = the library pow, 1 = exp2(alpha * log2(1 - x)) with
 * the logarithm in double + float parts, as the alpha sweep computes GD = (1 - D)^alpha (src/divergence.jl:142-148) */
int cge_pow_test(void *ctx, const double *x, int64_t n, double alpha, int method, double *out);
/* kernel-level hook (needs the GPU): vect_B, the community-pair sums of P_ij = (Ta_i Tb_j) GD_ij (src/divergence.jl:226-234,
 * :530-538), by ONE named form of the alpha sweep -- the sweep's own layout decision, tables and launch wrappers -- and the
 * divergence of the result from vC by the device-side mode selection.
 *   A problem: GD (N x N, row-major; the undirected forms read j >= i only), Ta, Tb (N; undirected callers pass one vector
 *   twice), comm (N ids in 1..C, any vertex order, ids without a member allowed), optional vC (the vector's length).
 *   vectB receives the vector (packed C (C + 1) / 2 undirected, C C directed) followed by CGE_VECT_B_GUARD doubles that sat
 *   behind it on the device and must still be NaN.  With vC: js_dev[3] = k_js modes 0 (all bins), 1 (internal), 2 (external)
 *   over the computed vector; forms 5 and 6 also give js_fused[n_modes] (n_modes 1: all bins; 2: internal, external) = the
 *   block partials of the one-launch form added in block order, then halved, as the sweep's host does (js_fused may be NULL).
 *   GD == NULL ("JS only", form 0): vectB is an input of the vector's length and only js_dev is computed.
 * form 0: what a sweep of this shape picks with the context's options (landmarks != 0: a landmark-mode sweep, else exact mode);
 *      1: staged row bins; 2: plain gather; 3: contiguous rows of the relabelled graph; 4: tiles + bins; 5: tiles + the bins
 *      and the divergence in one launch; 6: tiles + the batch's bins / JS launches over two problems, p and p2 (p2->C < p->C;
 *      p2 is read by this form only); 7: directed, tiles + bins on the PACKED tiles (GD, which must be symmetric, packed on the
 *      host through cge_packed_index; bvec_tile_dir_packed_kernel: a workgroup per stored tile writes its partials and its
 *      mirror tile's, at the positions and with the bits of form 4 directed).  *form_ran = the form that ran.  A relabelled form permutes GD, Ta, Tb and comm by the
 *      layout's order on the host, as the sweep computes GD from permuted rows.
 * CGE_E_ARG, with a message and before any launch, where the form does not apply: form 1 with N > 8192; forms 4-6 with
 * N < 256, C < 2 or more than 64 community ids in a 64-vertex block of the relabelled graph (form 7 too); forms 5, 6 directed;
 * form 7 undirected.
 * Not covered here: forms 4-6 make the tile partials by bvec_tile_kernel on a supplied GD; the partials a landmark-mode sweep gets
 * from the epilogue of its fused fit are cge_fused_chain_test's. */
#define CGE_VECT_B_GUARD 64
typedef struct cge_vect_b_problem {
    const double *GD, *Ta, *Tb;
    const int64_t *comm;
    int64_t N, C;
    const double *vC;
    double *vectB, *js_dev, *js_fused;
} cge_vect_b_problem;
int cge_vect_b_test(void *ctx, const cge_vect_b_problem *p, const cge_vect_b_problem *p2, int directed, int form, int landmarks,
                    int n_modes, int *form_ran);
/* kernel-level hook (needs the GPU): ONE Chung-Lu fit (src/divergence.jl:150-168, directed :434-467) from a caller's start, by
 * one named form of the alpha sweep -- the sweep's own fit functions, launch wrappers and geometry decisions -- so that a test
 * sees the iterate itself and the iteration count, not a score.
 *   A problem: D (N x N, row-major, symmetric, values in [0, 1]) and alpha: the fit reads GD = (1 - D)^alpha, made by
 *   k_pow_prepare + k_pow_matrix under the context's option "pow_exp2" (the fused forms 4 and 5 make it in their prologue from
 *   the tile-blocked logarithm).  The undirected forms read D on and above the diagonal 64 x 64 tiles only: j >= i, and the part
 *   of each diagonal tile below the diagonal (the tiles are read whole); every other element of D may hold anything.  The
 *   directed forms read all of it.
 *   w (N): the vertex weights (undirected) / deg_in (directed); w2 (N): deg_out (directed only).  T0 (N): the start T
 *   (undirected) / Tin (directed); T0b (N): the start Tout (directed only).
 *   Out: T, Tb (N; Tb directed only) = the iterate the fit left, copied from the device buffer the fit writes.  Undirected: that
 *   buffer holds NaN before the launch, so rows nothing wrote stay NaN (all of them after an abandoned launch).  Directed: the
 *   fit updates Tin / Tout in place on success only, so an abandoned launch returns the start.  GD (optional, N x N): the power
 *   matrix by k_pow_prepare + k_pow_matrix (undirected: the upper tiles; NaN where nothing was written).  iters = the
 *   iterations taken (iters updates were applied; the change f of the last one is <= delta); status = 0 converged, 1 the
 *   persistent launch was abandoned (context option "fit_persistent_test_timeout", or a wait that timed out).
 *   eps, delta: the step and the stopping threshold (a sweep: 0.25 / 0.001 undirected, 0.9 / 0.001 directed); the directed
 *   diff starts at 1.0 (:435).  The launch-per-iteration forms stop with CGE_E_ASSERT beyond option "fit_max_iterations".
 * form 0: what an exact-mode sweep of this shape picks on this device (the persistent form reading GD from 128 vertices on
 *         where its geometry applies, else one launch (pair) per iteration; an abandoned persistent launch is redone by launches,
 *         as the sweep does);
 *      1: one launch (pair) per iteration -- undirected fit_symtile_kernel + fit_symreduce_kernel over the upper tiles, directed
 *         fit_symv_dir_kernel + fit_update_dir_kernel;
 *      2: undirected, the same on the packed tiles (GD packed on the host through cge_packed_index, zeros outside the matrix);
 *      3: persistent, reading GD (fit_flow_kernel / fit_flow_dir_kernel);
 *      4: undirected, the fused instance of fit_flow_kernel without an epilogue output (needs option "pow_exp2");
 *      5: undirected, fit_flow_multi_kernel over n_problems (1..CGE_BATCH_MAX = 16) problems with slots and flags of their own.
 *      6: directed, fit_flow_dir_multi_kernel over n_problems (1..16) problems with slots, start vectors and flags of their
 *         own, each on the geometry (G, NW) of its own form-3 launch; per problem the outputs are form 3's: T, Tb, iters, status
 *         (an abandoned launch returns every member's start).
 *      7: directed, one launch pair per iteration by the tile kernels (fit_symtile_dir_kernel<false> + fit_symreduce_dir_kernel)
 *         on the row-major GD: every upper tile read once for Sin and Sout of both its blocks, the iterates alternating between
 *         two buffers, f in a ring of four and epsilon in a ring of two;
 *      8: directed, the same on the packed tiles (GD packed on the host through cge_packed_index); the bits of form 7.
 *      *form_ran = the form that ran.  n_problems > 1: form 5 (undirected) and form 6 (directed) only.
 * CGE_E_ARG, with a message and before any launch, where a form does not apply: forms 3-6 where the geometry of the persistent
 * fit declines N on this device; forms 2, 4, 5 directed; forms 6, 7, 8 undirected; forms 4, 5 without "pow_exp2"; forms 5, 6 with
 * problems of different waves per workgroup, more workgroups in all than the device has CUs or more than 16 problems; form 6
 * with a problem whose workgroups would reduce two quarter blocks each (the multi kernel exists for one).
 * Not covered here: forms 4 and 5 ask nothing of the fused launch's epilogue; its vect_B half and the tallies beside it are
 * cge_fused_chain_test's. */
typedef struct cge_fit_problem {
    const double *D, *w, *w2, *T0, *T0b;
    double *T, *Tb, *GD;
    int64_t N;
    double alpha;
    int64_t iters;
    int32_t status, pad;
} cge_fit_problem;
int cge_fit_test(void *ctx, cge_fit_problem *problems, int n_problems, int directed, int form, double eps, double delta, int *form_ran);
/* kernel-level hook (needs the GPU): the local half of the score (elements 5-7, src/divergence.jl:178-213, :485-517) stage by
 * stage -- the device sampler, the prepared pairs, full_graph_D of the sampled pairs and the tallies -- on the resident graph,
 * embedding and a caller's landmark data, by the sweep's own functions and launch wrappers.  A struct of optional stages: an
 * output that is NULL is not copied out, and a stage none of whose outputs is wanted and that no later stage needs is not run.
 * Every id is 0-based, as the device holds it.  S samples (all stages).
 *   Draw (draw_route 1: k_draw_samples_dev; 2: k_draw_samples_begin, then k_draw_samples_finish; 0: no draw) from seed and
 *   stream_id over the resident graph WHATEVER ITS SIZE (a score draws on the device beyond n (n - 1) = 2^25 only; that rule is
 *   the library's and stays).  Out: pos[S] (rows of the resident edge list), neg_i[S], neg_j[S], attempt[S] = the attempt number
 *   that gave each non-edge (the sampler's samp_attempt), *rounds = rounds of the rejection that ran.
 *   Prepare (k_prep_samples over the resident edge list) from pos_in / neg_i_in / neg_j_in, or the pairs just drawn where
 *   pos_in == NULL; pos2_in (optional): the overwriting draw of :510 -- the pairs come from pos2_in, the weights from pos_in.
 *   Out: pi, pj, ni, nj [S], wts[S].
 *   Distances (sampled_pair_dist on the resident embedding, divided by `hi`) of the prepared pairs, or of pi_in, pj_in, ni_in,
 *   nj_in (with wts_in, in place of Prepare).  Out: dpos[S], dneg[S].
 *   Tally (form != 0) over the prepared or supplied pairs and weights; dpos_in / dneg_in stand in for the distance stage, so a
 *   caller decides every tie.  Out: part[2 x 64] = the block tallies {num, den} and out2[2] = their sums in block order.
 *     form 1: k_auc_landmark on Ta, Tb (N; Tb == NULL: Ta), v2l[n], vw[n], lweight[N], alpha; out2 by auc_final_kernel.  old2new
 *             (optional, N): Ta / Tb are stored in sweep order (T[old2new[l]] belongs to landmark l) and un-permuted by
 *             k_permute_rows first, as local_score_tallies does;
 *     form 2: k_auc_exact on GD (N x N, row-major), Ta, Tb; the pairs index the N score-graph vertices;
 *     form 3: the same on the packed tiles (GD packed on the host through cge_packed_index; undirected: i <= j);
 *     form 5: k_auc_exact on the packed tiles with ORDERED pairs, as a packed directed sweep tallies them (GD, symmetric, packed
 *             on the host as for form 3; i > j allowed: a pair below the diagonal tiles reads the stored mirror); directed or not;
 *     form 4: the epilogue of the fused persistent fit, launched as enqueue_alpha launches it with the tally wanted and vect_B
 *             not: tables by fused_tables / k_auc_prepare (through old2new when given), the fit of cge_fit_test form 4 on D (N x N),
 *             w, T0 (sweep order), alpha, eps, delta.  Also out: T[N] = the iterate the launch left, aidx[4 S], afac[8 S],
 *             aden[64] as prepared, iters, status (1: the launch was abandoned -- part stays NaN); out2 is added on the host in
 *             block order, as the sweep's host does.
 *   sharded (default 0): a context whose rows or edges are sharded over ranks (options shard_rows / shard_ingest with collectives
 *   set) is refused.  sharded = 1 opts in: Draw, Prepare and Distances then run COLLECTIVELY -- every rank calls with the same
 *   arguments -- through the same wrappers, which dispatch to the exchange variants (collect_hit_kernel / check_neg_flag_kernel
 *   and the flag all-reduce of a round, prep_lookup_sharded_kernel / prep_store_sharded_kernel, pair_dist_rows_kernel behind the
 *   row exchange of sampled_pair_dist).  Every id stays GLOBAL: pos and pos_in / pos2_in are rows of the caller's whole edge
 *   list (range-checked against the total count, not this rank's share), pair ids are vertices, and every rank receives the
 *   full outputs.  A check that fails does so on every rank alike (the arguments are the same), before the first exchange.  The
 *   Tally forms stay refused on a sharded context, with or without the flag.  On a context that is not sharded the flag does
 *   nothing.
 * CGE_E_ARG with a message, before any launch: S < 1, a missing resident (graph for Draw / Prepare, embedding for Distances), a
 * context with option shard_rows or shard_ingest (unless sharded = 1 and form == 0), a row of pos_in / pos2_in outside the edge
 * list, a pair id outside the vertices (the landmark forms and the distances: n; forms 2, 3: N, and N = n on prepared pairs), v2l or old2new outside
 * 0..N-1 or old2new not a permutation, a stage without its inputs or with two sources of them, hi <= 0, N outside 1..46340,
 * forms 3, 4 directed, form 4 with eps <= 0 or delta < 0, without option "pow_exp2" or where the geometry of the fused fit
 * declines N.  The draw itself returns CGE_E_ARG ("could not find enough non-edges") when a sample is still an edge after 64
 * rounds; the context stays usable.
 * The exchange variants of options shard_rows / shard_ingest (pair_dist_rows_kernel, prep_*_sharded_kernel, collect_hit_kernel,
 * check_neg_flag_kernel) need a communicator: tests/test_gpu_ranks_small.py drives them through `sharded` on 2, 3 and 5 ranks.
 * Not covered here: the tallies split over ranks (tests/test_gpu_two_ranks.py and the whole-run cases of
 * tests/test_gpu_ranks_small.py hold them through the score); the multi-problem launch shares the
 * epilogue body and tests/test_gpu_batch.py holds its members to the single launch bit for bit; form 4 asks for the tally alone
 * -- the epilogue's vect_B, alone or beside the tally, and the multi-problem launch on supplied operands are
 * cge_fused_chain_test's. */
typedef struct cge_local_score_io {
    int64_t S, seed, stream_id;
    int32_t directed, draw_route, form, sharded;
    /* Draw */
    int32_t *pos, *neg_i, *neg_j;
    uint32_t *attempt;
    int64_t rounds;
    /* Prepare */
    const int32_t *pos_in, *pos2_in, *neg_i_in, *neg_j_in;
    int32_t *pi, *pj, *ni, *nj;
    double *wts;
    /* Distances */
    const int32_t *pi_in, *pj_in, *ni_in, *nj_in;
    const double *wts_in;
    double hi;
    double *dpos, *dneg;
    /* Tally */
    const double *dpos_in, *dneg_in;
    int64_t N;
    double alpha;
    const double *Ta, *Tb, *vw, *lweight, *GD;
    const int32_t *v2l, *old2new;
    double *part, *out2;
    /* form 4 */
    const double *D, *w, *T0;
    double eps, delta;
    double *T, *afac, *aden;
    int32_t *aidx;
    int64_t iters;
    int32_t status, pad2;
} cge_local_score_io;
int cge_local_score_test(void *ctx, cge_local_score_io *io);
/* kernel-level hook (needs the GPU): ONE alpha of the fused chain of an undirected landmark-mode sweep on a caller's problem -- the
 * launch of fit_flow_kernel<.., FUSED = true> (one problem) or fit_flow_multi_kernel (2 .. 16 problems) with its epilogue's
 * outputs wanted, then the bins and the divergence -- through the sweep's own functions: layout_tables (landmarks), community_tables,
 * k_bins_prepare, the epilogue table of fused_tables, k_pow_prepare (blocked), fit_undirected / the shared launch's table entry and
 * k_fit_flow_multi, k_bins_js / k_bins_js_multi.  So a test sees the tile partials themselves, bin by bin, not a score.
 *   A problem, in: D (N x N, row-major, symmetric, values in [0, 1]), w, T0 (N), alpha; comm (N ids in 1..C, any vertex order, ids
 *   without a member allowed); want (bit 0: vect_B's tile partials, bit 1: the tallies); vC (optional, packed C (C + 1) / 2) with
 *   n_modes (1: all bins; 2: internal, external).  With want bit 1 the prepared operands of the tally, as k_auc_prepare leaves
 *   them but the caller's: S in 1..65535, aidx[4 S] = indices into T in the caller's numbering (mapped through the layout's
 *   old2new here), afac[8 S], aden[64], dpos[S], dneg[S], wts[S].  D, w, T0 and comm are permuted by the layout's order on the
 *   host, as cge_vect_b_test permutes GD.  eps, delta: the step and the stopping threshold of every problem.
 *   Out: T[N] = the iterate the launch left, in the caller's numbering (NaN after an abandoned launch); iters; status (1: the
 *   launch was abandoned); order[N] = the layout's order (the 0-based vertex at each position of the sweep's numbering); the tile
 *   tables as the device holds them, fc[Nt], ns[Nt], base[Nt Nt], and bt_total; partials[bt_total] (partials_cap = the doubles
 *   the caller's array holds) copied out after the fit and before the bins -- [0, bt_total) is filled with NaN after
 *   k_bins_prepare and before the launch, so a partial nothing wrote stays NaN; vectB = the packed vector followed by
 *   CGE_VECT_B_GUARD doubles that sat behind it on the device and must still be NaN (want bit 0 of a converged launch; else all
 *   NaN); js_fused[n_modes] (with vC) = the block partials added in block order, then halved, as the sweep's host does;
 *   part[2 x 64] = the block tallies {num, den} (NaN unless the epilogue wrote them); apw[2 S] = the two powers per sample the
 *   launch's prologue made.  Every output pointer but T may be NULL.
 * Options the hook sets on the context (fit_fused, exact_relabel, test_bvec_plain, fit_persistent) are restored on the way out.
 * CGE_E_ARG with a message, before the fit is launched (the layout's refusals: behind the upload of its tables): a directed
 * call; N < 256 or C < 2; a context without option "pow_exp2" or one that gave the persistent fit up; a size whose geometry is not
 * that of the fused fit on this device; a layout that declines the tiles (more than 64 community ids in a 64-vertex block) or the
 * fused form (more than CGE_FLOW_NP = 32 pieces in a block), the message says which; want == 0 or beyond 3; want bit 1 without
 * its operands, S outside 1..65535 or an index outside 0..N-1; partials_cap below bt_total; several problems of different waves
 * per workgroup, with more workgroups in all than the device has CUs, or more than 16 of them; eps <= 0 or delta < 0.
 * Not covered here: the directed shared launch (cge_fit_test form 6), the tallies split over ranks and the packed exact sweep. */
typedef struct cge_fused_chain_problem {
    const double *D, *w, *T0;
    const int64_t *comm;
    int64_t N, C;
    double alpha;
    const double *vC;
    int32_t want, n_modes;
    int64_t S;
    const int32_t *aidx;
    const double *afac, *aden, *dpos, *dneg, *wts;
    double *T;
    int32_t *order, *fc, *ns, *base;
    double *partials;
    int64_t partials_cap, bt_total;
    double *vectB, *js_fused, *part, *apw;
    int64_t iters;
    int32_t status, pad;
} cge_fused_chain_problem;
int cge_fused_chain_test(void *ctx, cge_fused_chain_problem *problems, int n_problems, int directed, double eps, double delta);
/* kernel-level hook (needs the GPU): the packed form of an exact sweep (cge_hip.h, option "exact_packed") on a caller's
 * embedding, through the sweep's own launch wrappers -- the extrema pass (lo_hi[0], lo_hi[1] = extrema of D over j >= i with
 * diag on the diagonal, D never stored) and the generator of one alpha (distances, normalisation, power; pow_method 1 = exp2 of
 * the logarithm, 0 = the library pow).  The upper tiles are unpacked on the host through the address inline every consumer uses:
 * GD (N x N, row-major) is written for j >= i and, inside the diagonal 64 x 64 tiles, for j < i too (those tiles are stored
 * whole); the rest of each row is left as the caller filled it.  Any N >= 1 (the N >= 256 rule belongs to the sweep).
 * CGE_E_ASSERT when a tile element outside the matrix is not 0 */
int cge_packed_gd_test(void *ctx, const double *emb /* N x d row-major, host */, const double *diag /* N */, int64_t N, int64_t d,
                       double alpha, int pow_method, double *lo_hi /* 2 */, double *GD /* N x N row-major, host */);
/* kernel-level hook (needs the GPU): the SET-UP of an alpha sweep on a caller's score graph -- everything the per-alpha kernels
 * read, made once per sweep -- through the sweep's own functions and launch wrappers: edge_degrees (k_edge_degrees, into the
 * context's degree buffers), plan_layout (layout_tables, k_permute_rows, k_permute_i32), prepare_distances (k_dist_matrix,
 * k_minmax_upper, k_normalise, community_tables, the start vectors and TT), k_pow_prepare and k_pow_matrix, on the buffers a sweep
 * keeps them in.  The hook runs NO fit and no alpha.  A struct of optional stages: an output that is NULL is not copied out, and a
 * stage none of whose outputs is wanted and that no later stage needs is not run (the layout always runs: every later stage
 * reads it).
 *   In: emb (N x d, row-major), dist (N, the diagonal of D), comm (N ids in 1..C, any order, ids without a member allowed), vw
 *   (N, optional); directed; landmarks (a landmark-mode sweep: it decides the tile rule of the layout and whether form 0 keeps
 *   the upper tiles only); force_relabel (as cge_vect_b_test form 3 passes it to the layout); log_form 0 = what a sweep of this
 *   shape prepares, 1 = row-major whole, 2 = row-major upper tiles, 3 = tile-blocked; alpha (read when GD is wanted); an optional
 *   directed edge list src, dst (m 0-based ids), w (NULL = unit weights).  A directed call needs the edge list: its degrees set
 *   the start vectors.
 *   Degrees (with an edge list): deg_out[N], deg_in[N], star[N] (the rows of the edge list a vertex appears in, a self-loop
 *   twice).  This pass adds doubles with float atomics: for inexact weights its sums depend on the order the hardware serves the
 *   adds in (any order of a vertex's k terms: within (k - 1) 2^-53 sum|w| of the exact sum), for unit and dyadic weights every
 *   partial sum is exact and so is the result.  The line "no float atomics" at the top of kernels_fit.hip speaks of that file's
 *   reductions; it extends neither to this pass nor to the scatters of the landmark graph.
 *   Layout: relabel (0 / 1); order[N] and old2new[N] as the device holds them (written for a relabelled sweep only); emb_rl
 *   [N x d], vec_rl[4][N] = dist, vw, deg_in, deg_out (each where given), comm_rl[N] (0-based) = the per-vertex arrays the sweep
 *   goes on with -- the permuted copies, or the inputs themselves where the layout does not relabel; cm_off[C + 1], cm_mem[N],
 *   cm_pos[N] = the community tables as the device holds them.
 *   Distances: D_raw[N x N] = D as k_dist_matrix stores it (a launch of its own, before prepare_distances makes it again);
 *   lo_hi[2]; D[N x N] after the normalisation.
 *   The logarithm: Lh (doubles) and Ll (floats), log_cap elements each at the caller, in the layout that ran: log_form_ran (0:
 *   none -- option "pow_exp2" is off or there is no room; nothing is copied) and log_count, its elements (N N row-major,
 *   Nt (Nt + 1) / 2 x 4096 blocked).  Both device arrays hold NaN before the launch, so an element nothing wrote stays NaN.
 *   GD[N x N] (optional) by k_pow_matrix at alpha from what was prepared (the upper tiles alone after form 2), NaN where nothing
 *   was written; not written after form 3, which k_pow_matrix cannot read.
 *   Start: T1[N], T2[N] (undirected: ones; directed: Tin, Tout -- zero where the in- / out-degree is); TT[3 Tld] with Tld =
 *   64 ceil(N / 64): part 0 holds T1, everything else is zero.
 * CGE_E_ARG with a message, before any launch: N outside 1..46340, d < 1 or C < 1, a missing emb / dist / comm, a community id outside 1..C, an edge
 * endpoint outside 0..N-1, a directed call without edges, log_form outside 0..3, log_form 1-3 on a context without option
 * "pow_exp2", log_form 3 with N < 256, log_cap below the form's elements, a context with option shard_rows or shard_ingest; and,
 * behind the degree pass and the upload of the layout's tables (the verdict is the layout's own), log_form 3 where the layout
 * declines the tiles.  The hook sets no option.
 * Not covered here: the packed form of an exact sweep, which never stores D (cge_packed_gd_test has it), and the sharded set-up
 * (the whole runs of tests/test_gpu_two_ranks.py and tests/test_gpu_ranks_small.py). */
typedef struct cge_sweep_setup_io {
    const double *emb, *dist, *vw;
    const int64_t *comm;
    int64_t N, d, C;
    int32_t directed, landmarks, force_relabel, log_form;
    double alpha;
    const int32_t *src, *dst;
    const double *w;
    int64_t m;
    /* Degrees */
    double *deg_out, *deg_in;
    int32_t *star;
    /* Layout */
    int32_t *order, *old2new, *comm_rl, *cm_off, *cm_mem, *cm_pos;
    double *emb_rl, *vec_rl;
    /* Distances */
    double *D_raw, *lo_hi, *D;
    /* The logarithm and the power */
    double *Lh;
    float *Ll;
    int64_t log_cap, log_count;
    double *GD;
    /* Start */
    double *T1, *T2, *TT;
    int64_t Tld;
    int32_t relabel, log_form_ran;
} cge_sweep_setup_io;
int cge_sweep_setup_test(void *ctx, cge_sweep_setup_io *io);
/* needs the GPU and a communicator (cge_comm_init_rccl; one rank is enough): host array -> device -> the in-library
 * ncclAllReduce (op 0 sum / 1 max of doubles, 2 sum of the words as int64) -> host */
int cge_rccl_selftest(void *ctx, double *host_inout, int64_t count, int op);
/* kernel-level hook (needs the GPU): the per-group ascending STABLE sort of the projections as runsplit calls it (LDS pieces
 * + rank merge for long groups, rocPRIM otherwise): group t = rows [task_row_off[t], task_row_off[t+1]) of z; zs_out = sorted
 * values, perm_out[j] = index INSIDE its group of the element at sorted position j.  Order: ascending, -0.0 == 0.0, ties by
 * index (a group with NaNs is routed to the host path by its status) */
int cge_segment_sort_test(void *ctx, const double *z, const int32_t *task_row_off, int64_t T, double *zs_out, int32_t *perm_out);
/* kernel-level hook (needs the GPU): per row of 64 doubles, lane 0's sum by the shuffle tree (out_ref) and by the gfx950
 * lane swaps the projection kernel uses instead (out_new): the same pairs in the same order, so the same bits */
int cge_wave_tree_test(void *ctx, const double *x, int64_t n_rows, double *out_ref, double *out_new);
/* testing knobs of a context (needs the GPU; results must not depend on them):
 *   "fit_persistent_test_delay"   n: the tile waves of the persistent fits nap n x ~3 us before their first load (start skew, as
 *                                 under contention);
 *   "fit_persistent_test_timeout" 1: the persistent fit abandons every launch at once (the fallback path runs);
 *   "test_bvec_plain"             1: vect_B by the kernels of score graphs beyond the LDS budget / 512 communities;
 *   "fit_dir_tiles"               1: a resident directed launch-per-iteration fit goes by the tile pair (cge_fit_test form 7)
 *                                 instead of fit_symv_dir_kernel + fit_update_dir_kernel: the comparator of the packed directed sweep;
 *   "exact_resident_limit"        b: b bytes replace the 200e9 of the resident exact sweep's guard, so that the auto rule of
 *                                 option "exact_packed" and the CGE_E_OOM refusal can be driven at a few hundred vertices (0: the
 *                                 default).  This one does change which form runs;
 *   "louvain_wave_len"            l: levels >= 2 of cge_louvain_levels decide the vertices whose adjacency segment is longer than
 *                                 l by one wave each (-2: the default length, -1: every vertex, 2^31 - 1: none, the lane form alone);
 *   "test_rss2_one_kernel"        1: rss2 by the one-kernel walk (rss2_walk_kernel) at every width, d <= 128 included, where the
 *                                 chain + merge form runs otherwise: the two forms give the same bits;
 *   "test_eig_roles"              v: which wave of a workgroup of the batched eigen-solver (d <= 128) owns which column block and runs
 *                                 the tridiagonal tail: 0 (default) chosen by the waves' SIMDs, 1 the wave's number, 2 reversed,
 *                                 3 rotated by one: every choice gives the same bits;
 *   "test_pcent_form"             v: the form of the bf16-split bound pass of the pruned diameter: 0 (default) by the number of
 *                                 reference points, 1 the streaming form always, 2 the register-resident form wherever the
 *                                 pass applies (d <= 128): both forms give the same bits;
 *   "test_device_cus"             v: v in 1 .. the device's CU count replaces the CU count that sizes this context's launches: the
 *                                 geometry of the persistent fits (G, NW, NSB and whether they apply), the packing of
 *                                 cge_score_batch (max_G = v / 2), the slices of cge_link_topk / cge_link_rank and the grids of
 *                                 cge_link_sample / cge_link_auc; 0 (default): the device's own.  It only shrinks (above the count:
 *                                 CGE_E_ARG), since a persistent fit needs its G <= v workgroups co-resident.  This one does change
 *                                 which form runs -- on purpose: the forms of chips with fewer CUs run on a large one.  The link
 *                                 queries' results do not depend on it; a fit's agree to rounding;
 *   "test_lm_speculate"           v: which groups a round of runsplit's host driver (advance_heaps) puts into its batch -- and nothing
 *                                 else: which function computes the splits of a phase stays as it is.  0 (default): the global phase
 *                                 splits a share of the candidates per round, the forced phase the top of every local heap; 1: the
 *                                 global phase splits the top of its heap alone, the reference's own order, one split per round
 *                                 (stats "landmark_splits" == "landmark_pops": nothing wasted); 2: every candidate above the
 *                                 threshold is split, no `take` cut (a share of 100 %, the 512 rule of 64 < d <= 128 off); 3: as 0,
 *                                 and the forced phase's local heaps speculate too (target `forced`), the only way the speculating
 *                                 branch runs over more than one heap.  Other values: CGE_E_ARG.  The landmark ids and the errors are
 *                                 the same under every value; the stats "landmark_batches", "landmark_splits",
 *                                 "landmark_splits_failed" and "landmark_take_rounded" say what a value did.                        */
int cge_set_test_option(void *ctx, const char *key, int64_t value);
/* needs the GPU: the resident row-major fp64 matrix as this rank holds it (all n rows; under shard_rows its own rows, in
 * local order, with their global 0-based ids in ids_out, which may be NULL otherwise).  *rows and *d are set first; a capacity
 * below rows * d doubles (or a NULL out) returns CGE_E_ARG with them set, so a caller can ask for the sizes */
int cge_resident_embedding_test(void *ctx, double *out, int64_t capacity_doubles, int64_t *rows, int64_t *d, int32_t *ids_out);
/* needs the GPU: the resident graph and vertex data as this rank holds them, so that the tests of the graph views compare every
 * element and not a score.  The sizes come first (always set): n, m (edges held by this rank), unit (1 = an unweighted list: no
 * weights are kept), n_comm_max, n_comm16 (entries of the padded uint16 community table, 0 = none), have (bit 0 communities, bit
 * 1 vertex weights resident).  Every array pointer may be NULL (not copied); the capacities are in elements and a pointer whose
 * capacity is too small is CGE_E_ARG.  src / dst: m 0-based int32 ids; w: m doubles (not written for a unit list); comm: n
 * 0-based int32; comm16: n_comm16 entries; vweight: n doubles */
typedef struct cge_resident_graph {
    int64_t n, m, n_comm_max, n_comm16;
    int unit, have;
    int32_t *src, *dst, *comm;
    double *w, *vweight;
    uint16_t *comm16;
    int64_t cap_edges, cap_vertices, cap_comm16;
} cge_resident_graph;
int cge_resident_graph_test(void *ctx, cge_resident_graph *out);
/* needs the GPU: the member and peel stages of cge_ecg alone (members and seed as in cge_ecg_args, the same refusals).  members_out: members x n,
 * member r's partition renumbered 0 .. n_comm[r]-1 in ascending order of its labels, as a pass's is; rounds[r] and modularity[r]
 * go with it; core_out[v] = 1 where v is in the 2-core.  The stats "ecg_groups", "ecg_member_rounds", "ecg_peel_rounds" are set */
int cge_ecg_members_test(void *ctx, int64_t members, int64_t seed, int64_t *members_out, int64_t *n_comm, int64_t *rounds,
                         double *modularity, int32_t *core_out);
/* needs the GPU: cge_link_sample's launch with the uniform of a pair read from a caller-supplied n x n row-major matrix (n <= 1024)
 * in the place of the counter stream, so that a test can put every pair on its threshold at once: u(a, b) = U[a n + b] (0-based;
 * directed_layout = 0 reads U[min(a, b) n + max(a, b)], the upper triangle alone).  Everything else -- filter, exact evaluation,
 * sort, outputs, capacity rules, stats -- is cge_link_sample's */
int cge_link_sample_test(void *ctx, const double *U, int directed_layout, int64_t cap, int64_t *out_i, int64_t *out_j, double *out_p,
                         int64_t *n_edges);
/* needs the GPU: the matrix Q that cge_link_triangles' model half works on, generated by the same launch and copied out whole
 * (n <= 2048, undirected model): Q_out is ld x ld row-major with ld = 128 (ceil(n / 128) | 1), the library's own leading dimension
 * (another ld is CGE_E_ARG with the right one named).  Q[i ld + j] = min(cge_link_prob(i, j), 1) to the bit for i != j below n, 0
 * on the diagonal and in the padding */
int cge_link_triangles_test(void *ctx, double *Q_out, int64_t ld);
#ifdef __cplusplus
}
#endif
#endif
