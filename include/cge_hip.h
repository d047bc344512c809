/*
 * cge_hip.h -- C-ABI of libcge_hip.so: the MI355X (gfx950) implementation of CGE.jl's
 * divergence-scoring hot path.  This is the boundary a Julia `ccall`, a Python `ctypes`
 * or a C/C++ caller binds to.  Plain pointers and sizes only; no C++/torch types.
 *
 * What each entry point replaces in the reference (KrainskiL/CGE.jl v2.0.2):
 *   cge_landmarks_*      landmarks()        src/landmarks.jl:365-466  (+ runsplit :279-345, split rules :92-267)
 *   cge_wgcl             wGCL()             src/divergence.jl:27-257
 *   cge_wgcl (directed)  wGCL_directed()    src/divergence.jl:282-561
 *   cge_score            example/CGE_CLI.jl:4-24 (landmarks() followed by wGCL*() on device-resident data)
 *   cge_draw_samples     the `sample(E,..)` / `sample(NE,..)` draws, src/divergence.jl:184-210
 *   cge_js / cge_idx     JS() / idx()       src/auxilary.jl:34-52, :57-59
 *
 * Conventions (exactly the reference's, so a Julia Array can be passed as is):
 *   - vertex / community / landmark ids are 1-based int64;
 *   - matrices are column-major: edges (m x 2) = two contiguous int64 columns `src`,`dst`;
 *     an embedding (n x d) = d contiguous columns of n doubles;
 *   - host pointers are BORROWED for the duration of the call, never retained, never written
 *     (outputs excepted); outputs are caller-allocated;
 *   - every function returns an int status (0 = ok, <0 = error; cge_last_error() has the text);
 *     nothing throws or exits across the boundary;
 *   - a cge_ctx is bound to ONE GPU and is not re-entrant: one host thread drives it.
 *     Multi-GPU runs are one process (one ctx) per GPU; the cross-GPU exchange
 *     steps are issued by the library itself on an RCCL communicator (cge_rccl_unique_id +
 *     cge_comm_init_rccl: ncclAllReduce on the ctx stream), or, where no RCCL communicator can be
 *     made (gloo tests, two ranks on one GPU), go through the cge_collectives hook.
 *   - there is NO CPU fallback: without a gfx950 device cge_create fails with CGE_E_HIP.
 */
#ifndef CGE_HIP_H
#define CGE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGE_ABI_VERSION 1

/* status codes; the Julia wrapper maps them back to the reference's exceptions */
#define CGE_OK 0
#define CGE_E_ASSERT (-1)        /* an @assert of the reference (src/divergence.jl:50,81,303,363; src/landmarks.jl:93,...) */
#define CGE_E_HOMOGENEOUS (-2)   /* ErrorException("Trying to split homogenous cluster")  src/landmarks.jl:166 */
#define CGE_E_EMPTY_CLUSTER (-3) /* ErrorException("Unexpected empty cluster generated")  src/landmarks.jl:298,306,325,333 */
#define CGE_E_HIP (-4)           /* HIP runtime error / no device */
#define CGE_E_COLLECTIVE (-5)    /* a collective hook failed */
#define CGE_E_OOM (-6)
#define CGE_E_ARG (-7)           /* bad argument at the boundary */

/* split rule enum: the reference passes the function itself (src/auxilary.jl:64-67) */
#define CGE_METHOD_RSS 0
#define CGE_METHOD_RSS2 1
#define CGE_METHOD_SIZE 2
#define CGE_METHOD_DIAMETER 3

typedef struct cge_ctx cge_ctx;

/* ---- context ------------------------------------------------------------------------------ */
/* `stream`: a hipStream_t to launch on (NULL = the library creates its own).  Passing the host
 * framework's stream keeps its events/collectives ordered with the library's kernels.          */
int cge_create(cge_ctx **out, int device, void *stream);
void cge_destroy(cge_ctx *ctx);
const char *cge_last_error(const cge_ctx *ctx);
int cge_abi_version(void);
int cge_set_host_threads(cge_ctx *ctx, int n_threads); /* host worker pool for eigenvectors / cut rules */

/* Cross-GPU hooks (optional).  `buf` is a DEVICE pointer into the ctx's exchange buffer (obtain it
 * with cge_exchange_buffer and wrap it once on the host side); count is in doubles.  The hook must
 * order itself after work already enqueued on the ctx stream and leave the reduced data in place
 * (stream-ordered or synchronous).  op: 0 = sum, 1 = max, 2 = sum of the 8-byte words taken as
 * int64 (an exact gather of disjoint shards written into zero-filled buffers).                       */
typedef struct {
    int (*allreduce_f64)(void *user, void *buf, int64_t count, int op);
    void *user;
    int rank, world;
} cge_collectives;
int cge_set_collectives(cge_ctx *ctx, const cge_collectives *coll);
/* Further operations of the hook (optional; set AFTER cge_set_collectives, cleared by it): where they are present the library
 * moves gathers as gathers and the N x N landmark-pair matrix by row blocks instead of all-reducing whole buffers (what
 * ncclAllGather / ncclReduceScatter do on the in-library communicator).  Both work in place on `buf` (a device pointer into
 * the exchange buffer), `words` 8-byte words PER RANK, world * words in all:
 *   allgather(user, buf, words):          rank r contributes block [r * words, (r + 1) * words); afterwards every rank holds all;
 *   reduce_scatter_f64(user, buf, words): afterwards block r of rank r holds the sums (doubles) of that block over the ranks;
 *                                         the other blocks are unspecified.                                                  */
typedef struct {
    int (*allgather)(void *user, void *buf, int64_t words_per_rank);
    int (*reduce_scatter_f64)(void *user, void *buf, int64_t words_per_rank);
} cge_collectives_ext;
int cge_set_collectives_ext(cge_ctx *ctx, const cge_collectives_ext *ext);
int cge_exchange_buffer(cge_ctx *ctx, int64_t min_doubles, void **dev_ptr, int64_t *capacity_doubles);
/* or hand the library a caller-owned device buffer (e.g. a torch tensor) to use as exchange buffer */
int cge_set_exchange_buffer(cge_ctx *ctx, void *dev_ptr, int64_t capacity_doubles);

/* In-library collectives: RCCL over xGMI, one rank per GPU (csrc/collectives.cpp; librccl is opened at run time).  Rank 0
 * calls cge_rccl_unique_id and hands the CGE_RCCL_ID_BYTES bytes to every rank by whatever means the host has (MPI, a file,
 * torch.distributed); every rank then calls cge_comm_init_rccl on its context (collective: all ranks must call it).  From
 * then on the exchange steps of the path are ncclAllReduce calls issued by the library on the ctx stream -- no callback, no
 * host synchronisation per step, no exchange buffer to provide.  Takes precedence over a hook set with
 * cge_set_collectives.  cge_comm_finalize (also done by cge_destroy) releases the communicator.                       */
#define CGE_RCCL_ID_BYTES 128
int cge_rccl_unique_id(void *id_out);
int cge_comm_init_rccl(cge_ctx *ctx, const void *id, int rank, int world);
int cge_comm_finalize(cge_ctx *ctx);

/* ---- resident inputs (the ORIGINAL graph; uploaded once, H2D + layout change) ---------------
 * Calling cge_set_graph with another vertex count drops the resident embedding and vertex data (they were sized for the
 * old vertex set); cge_landmarks_run / cge_score check that all resident inputs agree and fail with CGE_E_ARG otherwise.
 * cge_wgcl in exact mode (empty v_to_l) makes ITS graph the resident one (the sampler rejects against it).
 * The ids are validated while they stream into the (already re-allocated) device arrays: a call that fails on a vertex id
 * outside 1..n leaves NO resident graph (the previous one is released, landmark state is invalidated); upload again.   */
/* src/dst: the two columns of the reference's `edges::Matrix{Int}` (src/auxilary.jl:106); w: eweights */
int cge_set_graph(cge_ctx *ctx, const int64_t *src, const int64_t *dst, const double *w, int64_t m, int64_t n);
/* embedding::Matrix{Float64} n x d column-major (src/auxilary.jl:164).  A shorthand for cge_set_embedding_view (below) of the view
 * {X_colmajor, d, ld = 0, CGE_DTYPE_F64, on_device = 0, row_major = 0}: there is one ingest, and this is one of its forms. */
int cge_set_embedding(cge_ctx *ctx, const double *X_colmajor, int64_t n, int64_t d);
/* The same for an embedding that already lives in THIS GPU's memory (a host framework's tensor; 41 GB at configuration 5
 * would otherwise cross PCIe): n x d doubles, row-major (row_major = 1: a vertex's d features contiguous) or column-major
 * like Julia's Matrix (0).  Copied (the caller keeps ownership and may free the buffer on return).  A shorthand for the view
 * {X_dev, d, ld = 0, CGE_DTYPE_F64, on_device = 1, row_major}; as for every device view, a pointer that is not device memory,
 * or that lies on another GPU than the context's (the kernels dereference it on the context's GPU), is CGE_E_ARG.        */
int cge_set_embedding_device(cge_ctx *ctx, const double *X_dev, int64_t n, int64_t d, int row_major);
/* The embedding AS THE CALLER HOLDS IT: fp64 / fp32 / fp16 / bf16 elements, in host memory or in this GPU's, row-major (a torch
 * tensor, a C-order numpy array) or column-major (Julia's Matrix), packed or with a leading dimension (a column slice X[:, :64] of a
 * wider matrix).  A host view crosses the link in its own type (half or a quarter of the fp64 bytes) and is widened on the device
 * behind each chunk of the upload; a device view is widened in one pass.  Widening to fp64 is exact, so the resident matrix holds,
 * bit for bit, what the caller's own conversion to double would have produced (signed zeros, subnormals and infinities included; a
 * NaN stays a NaN) and every result is that of cge_set_embedding / cge_set_embedding_device on the widened matrix.  Options
 * shard_rows / shard_ingest apply as they do to the fp64 forms (a device view is not ingest-sharded, as cge_set_embedding_device). */
#define CGE_DTYPE_F64 0
#define CGE_DTYPE_F32 1
#define CGE_DTYPE_F16 2   /* IEEE binary16 */
#define CGE_DTYPE_BF16 3
typedef struct {
    const void *data;   /* element (i, k): row-major data[i * ld + k], column-major data[k * ld + i] */
    int64_t d;          /* features */
    int64_t ld;         /* leading dimension in ELEMENTS; 0 = packed (d row-major, n column-major) */
    int dtype;          /* CGE_DTYPE_* */
    int on_device;      /* 0 host (borrowed for the call), 1 this GPU's memory (copied; caller may free on return) */
    int row_major;      /* 1 = a vertex's features contiguous; allowed for host pointers too */
} cge_embedding_view;
/* Is `v` a well-formed view of n rows?  Needs no context and no GPU.  CGE_E_ARG (and a message in `err`, optional) for a NULL view
 * or NULL data, d <= 0, n <= 0, an unknown dtype, a non-zero ld below the packed value, a data pointer that is not aligned to its
 * element size.  cge_set_embedding_view and cge_score_views call it first. */
int cge_embedding_view_check(const cge_embedding_view *v, int64_t n, char *err, int64_t err_len);
/* Makes the view the resident embedding (cge_set_embedding / cge_set_embedding_device are shorthands for it).  A device view whose
 * pointer is not device memory, or lies on another GPU than the context's (the kernels dereference it there): CGE_E_ARG. */
int cge_set_embedding_view(cge_ctx *ctx, const cge_embedding_view *v, int64_t n);
/* comm::Matrix{Int} n x 1 (src/auxilary.jl:122-139) and vweight (src/auxilary.jl:104-110).  A shorthand for cge_set_vertex_view
 * (below) of {comm, CGE_ID_I64, base 1, vweights, CGE_DTYPE_F64, host}, except that NULL vweights leave the resident ones. */
int cge_set_vertex_data(cge_ctx *ctx, const int64_t *comm, const double *vweights, int64_t n);

/* ---- graph views: the edge list and the vertex data AS THE CALLER HOLDS THEM ------------------------------------------------
 * What parseargs does to an edge file between `readdlm` and landmarks() (src/auxilary.jl:86-139), for arrays instead of text: a
 * PyG-style edge_index (2 x m, int32 or int64, 0-based, in GPU memory) is described in place, rebased, checked and narrowed by
 * the library, and vweight (the per-edge scatter of :104-110) and the clusters (:199-208) are derived from what is resident.
 * cge_set_graph / cge_set_vertex_data are shorthands for the views of their arguments: there is one ingest.                   */
#define CGE_ID_I64 0
#define CGE_ID_I32 1
typedef struct {
    const void *src, *dst;  /* endpoint of edge e: src[e * stride], dst[e * stride], in ELEMENTS */
    int64_t stride;         /* 1: two columns, or the two rows of a (2, m) tensor; 2: an (m, 2) C-order array (dst = src + 1); any value >= 1 */
    int id_dtype;           /* CGE_ID_* */
    int base;               /* 0 or 1; -1 = decided as parseargs does: the minimum id must be 0 or 1 (src/auxilary.jl:92-98) */
    const void *w;          /* eweights; NULL = an unweighted list (unit weights, :105) */
    int w_dtype;            /* CGE_DTYPE_F64 or CGE_DTYPE_F32 (widening is exact); F16 / BF16 are CGE_E_ARG */
    int on_device;          /* 0: host, borrowed for the call; 1: this GPU's memory, copied -- all pointers of a view in one place */
} cge_graph_view;
/* Is `g` a well-formed view of m edges?  Needs no context and no GPU.  CGE_E_ARG (and a message in `err`, optional) for a NULL
 * view, NULL src / dst, m <= 0, stride < 1, an unknown id or weight dtype (F16 / BF16 weights included), a base outside
 * {-1, 0, 1}, a pointer that is not aligned to its element, and src / dst ranges that overlap otherwise than as the two
 * interleaved columns their stride describes. */
int cge_graph_view_check(const cge_graph_view *g, int64_t m, char *err, int64_t err_len);
/* Makes the view the resident graph: afterwards the context holds, bit for bit, what cge_set_graph leaves for the same edges
 * given as 1-based int64 columns with fp64 weights (0-based int32 ids, the unit-weight verdict, the weights and their host
 * mirror), so every result downstream is the same.  n = 0: the number of vertices is the maximum id (:99); *n_out (optional)
 * receives it.  All checks are made on the 64-bit ids before they are narrowed and before anything is indexed by one:
 * base = -1 and a minimum other than 0 or 1 is CGE_E_ASSERT "Vertices should be either 0-based or 1-based" (:93); an id outside
 * the vertex range is CGE_E_ARG naming the lowest offending edge (1-based row).  After such an error NO graph is resident.
 * A device view is rebased, checked, narrowed and widened by kernels (only scalars, and the weights' host mirror of a weighted
 * list, come back); a pointer that is not memory of the context's GPU is CGE_E_ARG; it is not ingest-sharded (as
 * cge_set_embedding_device).  A host view goes through the staging workers of cge_set_graph, option shard_ingest included. */
int cge_set_graph_view(cge_ctx *ctx, const cge_graph_view *g, int64_t m, int64_t n /* 0 = maximum id, :99 */, int64_t *n_out);

typedef struct {
    const void *comm;       /* n community ids, or NULL (leave the resident ones) */
    int id_dtype, base;     /* as above; base -1 = minimum must be 0 or 1 (:133-139) */
    const void *vweights;   /* n vertex weights; NULL = DERIVE them from the resident edge list (:104-110) */
    int vw_dtype;           /* F64 / F32 */
    int on_device;
} cge_vertex_view;
/* comm (src/auxilary.jl:122-139) rebased, checked (>= 1 after rebasing, CGE_E_ARG otherwise; base = -1 and a minimum other than
 * 0 or 1: CGE_E_ASSERT "Communities should be either 0-based or 1-based", :134) and narrowed into the tables cge_set_vertex_data
 * builds.  vweights == NULL: vweight[v] = the weights of v's incident edges added in edge order starting from 0.0, an edge
 * counting for its source and then for its target (a self-loop twice in a row), i.e. the bits of the loop at :107-110; an
 * isolated vertex gets 0.0.  Needs the resident graph (of n vertices) whole on this rank: on an edge list sharded over the ranks
 * (option shard_ingest) the derivation is CGE_E_ARG -- a sum in edge order cannot be put together from per-rank partial sums. */
int cge_set_vertex_view(cge_ctx *ctx, const cge_vertex_view *v, int64_t n);
/* the resident vweight (n doubles), for callers of the reference-shaped entries (cge_wgcl takes vweights as an argument) */
int cge_vertex_weights(cge_ctx *ctx, double *out, int64_t n);

/* ---- landmarks(): src/landmarks.jl:365-466 --------------------------------------------------- */
/* clusters::Vector{Vector{Int}} as CSR: members clusters_flat[off[c] .. off[c+1]) (1-based ids).
 * Runs on the resident inputs; results stay on the device (for cge_wgcl / cge_score) and can be
 * fetched.  `*N_out` = number of landmarks, `*n_ledges_out` = rows of landmark_edges (w > 0),
 * `*truncated` = 1 when the reference's @warn at :374 would have fired.
 * n_clusters == -1 (here, in cge_runsplit and in cge_score_args): the clusters are DERIVED from the resident communities as
 * parseargs builds them (src/auxilary.jl:199-208) -- one cluster per community that occurs, members in ascending vertex id;
 * the two pointers are ignored (runsplit orders the clusters itself, so their order is immaterial).                        */
int cge_landmarks_run(cge_ctx *ctx, const int64_t *clusters_flat, const int64_t *clusters_off, int64_t n_clusters,
                      int64_t land, int64_t forced, int method, int directed, int64_t *N_out,
                      int64_t *n_ledges_out, int *truncated);
/* sizes of the landmark state produced by the last cge_landmarks_run / cge_score on this ctx */
int cge_landmarks_info(cge_ctx *ctx, int64_t *N_out, int64_t *n_ledges_out, int *truncated);
/* the reference's 7-tuple (src/landmarks.jl:465): dii[N], embed[N x d col-major], cluster[N],
 * landmark_edges[n_ledges x 2 col-major], weights[n_ledges], lweight[N], v_to_l[n]              */
int cge_landmarks_fetch(cge_ctx *ctx, double *dii, double *embed, int64_t *cluster, int64_t *ledges,
                        double *lweights_e, double *lweight, int64_t *v_to_l);
/* runsplit() alone (src/landmarks.jl:279-345): 0-based group ids, for parity tests              */
int cge_runsplit(cge_ctx *ctx, const int64_t *clusters_flat, const int64_t *clusters_off, int64_t n_clusters,
                 int64_t nland, int64_t forced, int method, int64_t *group_ids);

/* ---- local-score samples --------------------------------------------------------------------- */
/* Counter-based draws (documented in DESIGN.md; the Julia stream cannot be reproduced):
 * pos_idx[k] uniform in 1..m (rows of the original edge list, `sample(E,S,replace=true)`),
 * (neg_i,neg_j)[k] uniform over NON-edges of the resident graph (`sample(NE,S,replace=true)`),
 * by rejection against the resident edge list, i<j for undirected, ordered i!=j for directed.
 * `stream_id` selects an independent stream (the alpha index when the run is unseeded).          */
int cge_draw_samples(cge_ctx *ctx, int64_t seed, int64_t stream_id, int64_t S, int directed, int64_t *pos_idx,
                     int64_t *neg_i, int64_t *neg_j);

/* ---- wGCL() / wGCL_directed(): src/divergence.jl:27-31, :282-286 -------------------------------- */
typedef struct {
    /* the 15 reference arguments, pointer + length */
    const int64_t *edges_src, *edges_dst; /* edges (m x 2)                     */
    const double *eweights;              /* m                                  */
    int64_t m;
    const int64_t *comm;                 /* comm (N x 1)                       */
    int64_t n_comm;
    const double *embed;                 /* N x d column-major                 */
    int64_t embed_rows, d;
    const double *distances;             /* N                                  */
    int64_t n_distances;
    const double *vweights;              /* N                                  */
    const double *init_vweights;         /* n or empty                         */
    int64_t n_init;
    const int64_t *v_to_l;               /* n or empty (empty <=> exact mode, src/divergence.jl:44) */
    int64_t n_v_to_l;
    const int64_t *init_edges_src, *init_edges_dst; /* m_init x 2 or empty    */
    int64_t m_init;
    const double *init_eweights;
    const double *init_embed;            /* n x d column-major or empty        */
    int split;                           /* --split-global                     */
    int64_t seed;                        /* -1 = unseeded                      */
    int64_t auc_samples;
    int verbose;
    int directed;                        /* 0: wGCL, 1: wGCL_directed          */
    /* optional pre-drawn samples so the caller can own the RNG (n_sets = 1, or one set per alpha);
     * NULL => the library draws them with cge_draw_samples(seed, ...)                              */
    const int64_t *pos_idx, *neg_i, *neg_j, *pos_idx2;
    int64_t n_sample_sets;
} cge_wgcl_args;

/* per-alpha trace (optional, for parity tests and the bench's evaluation count)                 */
typedef struct {
    int64_t n_alpha;
    int64_t iters[64];
    double div[64];
    double auc[64];
} cge_trace;

/* Host-array form: uploads what it is given, runs on the GPU, returns the reference's vector:
 * [best_alpha, best_div, best_div_ext, best_div_int, best_alpha_auc, best_auc, best_auc_err]
 * (*out_len = 7; 6 for the directed star-graph early return, src/divergence.jl:332-334).          */
int cge_wgcl(cge_ctx *ctx, const cge_wgcl_args *args, double out[7], int *out_len, cge_trace *trace);

/* Device-resident form of example/CGE_CLI.jl:10-24: landmarks() on the resident inputs, then
 * wGCL*() in landmark mode, with no host round trip of the landmark graph.  land = -1 runs
 * the exact mode on the resident graph (distances = zeros, CGE_CLI.jl:4).  Exact mode -- here and in
 * cge_wgcl with an empty v_to_l -- keeps D, GD and the logarithm on the device (17.6 - 28 bytes per vertex pair) up to
 * N ~ 1.06e5 vertices; beyond, an UNDIRECTED sweep runs on the upper 64 x 64 tiles of the current alpha's GD alone
 * (~4.1 bytes per pair: N ~ 2.3e5 on a 288 GB card; option "exact_packed").  A DIRECTED exact sweep stays
 * resident and is refused beyond its limit (CGE_E_OOM; the message names option "exact_packed_directed") unless that option
 * allows it the same tiles (~4.25 bytes per pair: the model's matrix is symmetric, only Tin / Tout are not).  Refused too is a
 * sweep the packed form does not apply to or whose tiles do not fit the free memory (the message names N and the bytes).  */
typedef struct {
    const int64_t *clusters_flat, *clusters_off;
    int64_t n_clusters;
    int64_t land, forced;
    int method, directed, split;
    int64_t seed, auc_samples;
} cge_score_args;
int cge_score(cge_ctx *ctx, const cge_score_args *args, double out[7], int *out_len, cge_trace *trace);

/* cge_score for K embeddings of the resident graph in one call: member k's vector (out + 7 k, out_len[k] = 7, or 6 for the
 * directed star return) and trace (traces + k, optional) are what cge_score(args) gives on that embedding on this context with
 * the same options -- the same bits and iteration counts.  The graph and the vertex data must be resident; the resident
 * embedding is replaced member by member, and afterwards the resident embedding and landmark state are the LAST member's.
 * Undirected landmark-mode members on the fused persistent fit (>= 256 landmarks, options fit_fused = 1, fit_persistent != 1)
 * share their sweeps: the members' fits of an alpha run in ONE launch (launch groups of at most the CU count in workgroups,
 * run one after another), and so do their vect_B and JS; the local score's samples are drawn once.  DIRECTED landmark-mode
 * members share the fit alone: with >= 256 landmarks, fit_persistent != 1, a persistent directed fit of one quarter block per
 * workgroup on at most half the CUs (256 <= N <= 1984 on 256 CUs) and the row forms of vect_B (not bvec_blocks = 1), the
 * members' directed fits of an alpha run in ONE launch, each on the workgroups of its own launch; the power matrix, the local
 * score's tallies, vect_B and JS stay launches of their own per member.  Option fit_fused and the 65 536-sample limit of the
 * fused tallies do not apply to them.  While its launch group runs, a directed member holds 16 N^2 bytes (D and its power
 * matrix), 28 N^2 with the stored logarithm (pow_exp2).  Every other member (exact mode land = -1, fewer landmarks, a star
 * graph's early return) is scored on its own, as cge_score would.  Not under collectives or
 * sharding (CGE_E_ARG: one embedding per rank is the multi-GPU form).  On an error (e.g. CGE_E_HOMOGENEOUS of a member) the
 * call returns it with every out_len[k] = 0; the context stays usable.  Stats "fit_batched_launches" / "fit_batched_alphas":
 * multi-problem fit launches of the last call and the member-alphas they fitted.                                            */
typedef struct {
    const double *const *embeddings; /* K pointers, each n x d (the resident graph's n), one common d */
    int64_t K, d;
    int on_device;                   /* 0: host, column-major (as cge_set_embedding); 1: device (as cge_set_embedding_device) */
    int row_major;                   /* device pointers only: 1 = a vertex's d features contiguous */
} cge_embedding_batch;
int cge_score_batch(cge_ctx *ctx, const cge_score_args *args, const cge_embedding_batch *batch, double *out /* K x 7 */,
                    int *out_len /* K */, cge_trace *traces /* K or NULL */);
/* cge_score_batch with one view per member (of the resident graph's n rows): the members may differ in d, dtype, layout and
 * location -- a 32-dimensional fp32 tensor on the device can be ranked against a 64-dimensional fp64 host matrix.  The same
 * contract: member k's vector, trace and iteration counts are what cge_score gives after cge_set_embedding_view(views + k) on this
 * context; the same launch sharing, stats and error behaviour, the same refusal under collectives or sharding; afterwards the
 * last member is resident. */
int cge_score_views(cge_ctx *ctx, const cge_score_args *args, const cge_embedding_view *views, int64_t K,
                    double *out /* K x 7 */, int *out_len /* K */, cge_trace *traces /* K or NULL */);

/* ---- louvain_clust(): src/clustering.jl:14-68 (called by parseargs when `-c` is omitted, src/auxilary.jl:115-121) ----
 * The communities the reference writes to <file>.ecg: LEVEL 1 of Louvain (`hierarchy -l 1`: the partition after the first
 * pass of local moving), here computed on the resident graph (cge_set_graph; weights honoured) by synchronous rounds on
 * the device.  comm_out[v] (v = 0 .. n-1) in 0 .. *n_comm-1; *modularity = modularity of that partition.  The reference
 * visits the vertices in an unseeded random order, so partitions are comparable in quality, not in identity.            */
int cge_louvain(cge_ctx *ctx, int64_t *comm_out, int64_t *n_comm, double *modularity, int64_t *rounds);
/* The whole hierarchy.  The reference runs `louvain -l -1`, which computes every level, and `hierarchy -l 1` then keeps the
 * first (src/clustering.jl:20-24); here a caller may ask for level 2, 3, or the last.  Level L + 1 is the same pass on level
 * L's graph contracted by level L's communities (`partition2graph_binary`), and the hierarchy ends at the first level that
 * merges nothing; that level is not reported, except level 1, which always is and equals cge_louvain's result.  So every
 * reported level after the first has strictly fewer communities than the one before.
 * Row l of comm_out (levels_cap x n, level-major) = level l + 1's community of every ORIGINAL vertex, 0-based and consecutive;
 * n_comm[l], modularity[l] (of that partition on the resident graph), rounds[l] go with it.  *n_levels = the number of levels
 * the hierarchy has under max_levels (<= 0: until a level merges nothing).  levels_cap = 0 (every array may be NULL) asks for
 * that number alone; more levels than levels_cap > 0 is CGE_E_ARG, with *n_levels set and named in the message, and the first
 * levels_cap rows written.  Argument checks as cge_louvain: no resident graph, or a sharded edge list, is CGE_E_ARG.
 * On integer and dyadic weights every level is determined to the bit; on other weights only the quality is comparable.  */
int cge_louvain_levels(cge_ctx *ctx, int64_t max_levels /* <= 0: until a level merges nothing */, int64_t levels_cap,
                       int64_t *comm_out /* levels_cap x n, level-major; may be NULL with levels_cap 0 */, int64_t *n_levels,
                       int64_t *n_comm /* [levels_cap] */, double *modularity /* [levels_cap] */, int64_t *rounds /* [levels_cap] */);

/* ---- ECG communities (an extension; the reference ships *.ecg files made by Ensemble Clustering for Graphs, Poulin & Theberge) ----
 * `members` level-1 passes of cge_louvain's kind on the resident graph, member r under the vertex names rank_r (v ordered by
 * (mix(base_r ^ v), v), mix = splitmix64, base_r = mix(seed ^ mix(r))); the 2-core on adjacency entries (repeated edges are
 * separate entries, self loops are none); every edge reweighted  w_min + (1 - w_min) c / members  (c = members that put both its
 * ends in one community) when both ends are in the 2-core, w_min otherwise -- the graph's own weights drive the members and do not
 * enter these; then the Louvain hierarchy on the reweighted graph, of which level final_level (-1: the last; k >= 1: level k, or
 * the last of a shorter hierarchy) is returned.  comm_out[v] in 0 .. *n_comm-1; *modularity is that partition's on the resident
 * graph with its own weights, *modularity_ecg on the reweighted graph; edge_weights_out receives the new weight of every edge.
 * Departures from the published algorithm: the members are synchronous passes diversified by relabelling alone, and the 2-core
 * counts adjacency entries.  CGE_E_ARG with a message, before any device work: members outside 1 .. 64, w_min not in [0, 1) (or
 * NaN), final_level 0 or below -1; then as cge_louvain: no resident graph, a sharded edge list.  On integer and dyadic weights
 * with members and 1 / w_min powers of two everything is determined to the bit; with other values (the default w_min = 0.05)
 * the members still are (on such graph weights), but the final hierarchy runs on real weights, where -- as for cge_louvain_levels -- only the quality
 * is comparable and two calls may break a tie differently.  Results never depend on option "ecg_group".
 * Stats: "ecg_groups", "ecg_member_rounds" (summed over the members), "ecg_peel_rounds", "ecg_levels". */
typedef struct { int64_t members; double w_min; int64_t seed; int64_t final_level; } cge_ecg_args;
int cge_ecg(cge_ctx *ctx, const cge_ecg_args *args, int64_t *comm_out /* n, 0-based consecutive */, int64_t *n_comm,
            double *modularity /* original graph */, double *modularity_ecg /* reweighted graph, may be NULL */,
            double *edge_weights_out /* m, edge order, may be NULL */);

/* ---- link prediction under the fitted model (an extension) ---------------------------------------------------------------------
 * The local score, elements 5-7 of the result vector, is a link-prediction AUC of the geometric Chung-Lu model fitted at an alpha
 * (src/divergence.jl:178-213, directed :478-517).  These entry points keep that model and evaluate it on the caller's pairs:
 *     p(i, j) = f_out[i] * f_in[j] * max(0, 1 - dist(i, j) / hi) ^ alpha         (evaluated left to right as written)
 * with dist = src/auxilary.jl:14-20 in pair_dist_kernel's arithmetic (ascending k, one rounding per operation; dist(i, i) = 0), hi
 * the point-set diameter (lo = 0: the diagonal of D is 0, so (D - lo) / (hi - lo) = D / hi to the bit), and the factors
 *     landmark mode:  f[v] = T[l_v] * vw_v / lw[l_v]  (:187-188; directed: Tout into f_out, Tin into f_in, :488-489),
 *     exact mode:     f = T  (:174, :474).
 * A link model {directed, alpha, hi, f_out[n], f_in[n]} lives on the device beside the resident embedding and edge list it refers
 * to.  Every call that replaces the resident embedding, graph or vertex data (cge_set_embedding*, cge_set_graph*, cge_set_vertex_*,
 * cge_score_batch / cge_score_views, an exact-mode cge_wgcl) drops it; afterwards cge_link_model_fetch / cge_link_prob /
 * cge_link_topk answer CGE_E_ARG "no link model".  Not under collectives or sharding (CGE_E_ARG).
 * The power is taken in the form the sweep's local score used, so that the values have the bits its tallies compared: the library
 * pow in landmark mode (auc_landmark_kernel) and for a supplied model; in exact mode the per-element chain of the power matrix
 * (log2(1 - x) to ~70 bits, then exp2: option "pow_exp2", else the library pow).  The base is clamped at 0 (only a supplied hi
 * below the diameter can make it negative).  Undirected values are symmetric in (i, j).  A non-finite embedding is not supported:
 * its probabilities are NaN and cge_link_topk's lists are unspecified.                                                           */
#define CGE_LINK_BEST_LOCAL 1  /* the alpha of element 5 (best local score) */
#define CGE_LINK_BEST_GLOBAL 2 /* the alpha of element 1 (best divergence)  */
/* cge_score(args) that also keeps the model of one alpha.  out, out_len, trace, every stat and the iteration counts are what
 * cge_score gives on the same context with the same options, bit for bit: it is ONE sweep, and with no model wanted that sweep
 * enqueues exactly what it always did.  The kept T is the sweep's own iterate at that alpha (warm-started as the sweep warms it,
 * :118) -- the T the reported score was computed from -- copied aside on the stream when the alpha becomes the best of the wanted
 * kind; a relabelled sweep's T is un-permuted to the original numbering.  Afterwards the factors are expanded on the device and
 * hi is the value the sweep normalised by.  A directed star graph's early return (out_len = 6) leaves no model, and so does a
 * sweep that never recorded a best of the wanted kind.  CGE_E_ARG: under collectives or sharding (as cge_score_batch); `which`
 * other than the two values; CGE_LINK_BEST_LOCAL with auc_samples < 1.                                                          */
int cge_link_fit(cge_ctx *ctx, const cge_score_args *args, int which, double out[7], int *out_len, cge_trace *trace);
/* A caller-supplied model over the resident embedding and graph (f_in = NULL: f_in = f_out).  CGE_E_ARG, before any device work:
 * no resident embedding or graph; n other than the resident n; alpha or hi non-finite or <= 0; a negative or non-finite factor;
 * directed = 0 with an f_in of its own (an undirected model has one factor per vertex).                                          */
int cge_link_set_model(cge_ctx *ctx, int directed, double alpha, double hi, const double *f_out, const double *f_in /* NULL: = f_out */,
                       int64_t n);
/* The resident model; every output is optional.  f_out / f_in: n doubles each; T_out / T_in: the *N landmark (exact mode: vertex)
 * iterates of a fitted model in the original numbering (undirected: the same vector twice); *N = 0 for a supplied model.         */
int cge_link_model_fetch(cge_ctx *ctx, int *directed, double *alpha, double *hi, double *f_out, double *f_in, double *T_out,
                         double *T_in, int64_t *N);
/* out[q] = p(i[q], j[q]) for P >= 1 pairs of 1-based vertex ids (an id outside 1 .. n: CGE_E_ARG, before any device work).      */
int cge_link_prob(cge_ctx *ctx, const int64_t *i, const int64_t *j, int64_t P, double *out);
/* For every query i, in the order given (repeats allowed), the k candidates j != i of largest p(i, j), sorted by (p descending,
 * j ascending) -- ties go to the smaller j.  exclude_edges = 1 leaves out the vertices joined to i by a resident edge: undirected,
 * either orientation of the list counts; directed, only i -> j does (j -> i does not exclude); repeated edges and self loops
 * change nothing.  1 <= k <= 64 (else CGE_E_ARG; so is a query id outside 1 .. n, before any device work).  A query with fewer
 * than k admissible candidates gets out_cnt < k and 0 / 0.0 in the unused slots.  Every reported p is cge_link_prob's value for
 * that pair, bit for bit, and the ranking is by those values: the result is a function of the inputs alone, not of the grid, the
 * slicing of the candidates or the order of insertion.  (The kernel ranks nothing by the Gram formula: that only FILTERS, with a
 * rounding bound that keeps every pair that could belong)
 * Stats: "link_topk_survivors" = pairs of the last call that passed the filter and were evaluated exactly, "link_topk_queries".  */
int cge_link_topk(cge_ctx *ctx, const int64_t *queries, int64_t Q, int64_t k, int exclude_edges, int64_t *out_j /* Q x k */,
                  double *out_p /* Q x k */, int64_t *out_cnt /* Q */);
/* The exact filtered rank of P >= 1 given pairs (i[q], j[q]), 1-based ids, among the candidates of their source vertex -- what MRR,
 * Hits@K, mean rank and per-pair AUC are made of.  With p* = cge_link_prob's value of (i, j), bit for bit, and the admissible
 * candidates A = {c : c != i, c != j, and -- exclude_edges = 1 -- c not joined to i by a resident edge (cge_link_topk's rules:
 * undirected either orientation, directed i -> c alone; repeated edges and self loops change nothing)}:
 *     out_greater[q] = #{c in A : p(i, c) > p*},   out_ties[q] = #{c in A : p(i, c) == p*},   out_cand[q] = |A|,   out_p[q] = p*.
 * j itself is never removed from the question, even when (i, j) is a resident edge (a held-out edge is not resident; a resident
 * one is ranked against the non-neighbours).  Every p is cge_link_prob's value and the comparisons are made on those values (the
 * Gram formula only filters, as in cge_link_topk), so the result is a function of the inputs alone: not of the grid, the slicing,
 * the order of the pairs or the other pairs of the call.  Pairs may repeat.  Consistent with cge_link_topk: if j is admissible
 * there and sits at position r (0-based) of query i's list, then greater <= r <= greater + ties under the same exclude_edges.
 * CGE_E_ARG, before any device work: no link model; P < 1; an id outside 1 .. n; i[q] == j[q] (a vertex is not its own candidate);
 * under collectives or sharding.  A non-finite embedding is unspecified, as for cge_link_topk.  DESIGN.md section 4.12.
 * Stats: "link_rank_survivors" = (query, candidate) pairs of the last call evaluated exactly, "link_rank_queries" = its distinct
 * query vertices.                                                                                                                */
int cge_link_rank(cge_ctx *ctx, const int64_t *i, const int64_t *j, int64_t P, int exclude_edges,
                  int64_t *out_greater /* P */, int64_t *out_ties /* P */, int64_t *out_cand /* P, may be NULL */,
                  double *out_p /* P, may be NULL */);
/* One draw of the random graph the model IS: every pair is an edge independently with probability p(i, j).  The sampled set is
 *     {(i, j) : u(i, j) < p(i, j)},   u(a, b) = (cge_ctr_rand(seed, stream, a, b, 5) >> 11) * 2^-53   (a, b the 0-based ids),
 * with p cge_link_prob's value, bit for bit (a p >= 1 is always an edge), over the pairs i < j of an undirected model and over all
 * ordered pairs i != j of a directed one ((i, j) and (j, i) are independent draws).  No self loops; the resident edges play no
 * part.  cge_ctr_rand is the sampler's counter stream (splitmix64 rounds over seed, stream, a, b, which; which = 5 is this call's).
 * Output: 1-based ids, rows sorted by (i, j) ascending, out_p[e] the pair's p, *n_edges the size of the set.  The result is a
 * function of (model, embedding, seed, stream) alone: not of the grid, the slicing or the order of the appends.
 * cap = 0 (the arrays may be NULL) only counts.  A set larger than cap > 0 is CGE_E_ARG with *n_edges set (and named in the
 * message) and the arrays unspecified; the context stays usable and the same call with a sufficient cap gives the set.
 * CGE_E_ARG, before any device work: no link model; cap < 0; a NULL n_edges; cap > 0 with a NULL out_i / out_j; under collectives
 * or sharding.  A non-finite embedding is unspecified, as for cge_link_topk.  DESIGN.md section 4.13.
 * Stats: "link_sample_edges", "link_sample_survivors" = pairs of the last call that passed the filter and were evaluated exactly,
 * "link_sample_tiles".                                                                                                            */
int cge_link_sample(cge_ctx *ctx, int64_t seed, int64_t stream, int64_t cap, int64_t *out_i /* cap */, int64_t *out_j /* cap */,
                    double *out_p /* cap, may be NULL */, int64_t *n_edges);
/* The exact link AUC of the resident model on the resident graph: what elements 5-7 of a score estimate from auc_samples draws,
 * over ALL edges and ALL non-edges.
 *   Positives: the m rows of the resident edge list, in the list's order; a repeated row is a repeated positive (as the sweep's
 *              sampler draws them), a self loop is included with p(i, i) = f_out[i] * f_in[i] (dist(i, i) = 0).  p_e =
 *              cge_link_prob's value of row e, bit for bit (out_p).
 *   Negatives: NE, the pairs the sampler rejects against: undirected, the pairs i < j that no resident row joins in either
 *              orientation; directed, the ordered pairs i != j with no row i -> j.  No self pairs.  *n_neg = |NE|, from the
 *              distinct non-loop keys of the edge list.
 *     out_less[e] = #{(a, b) in NE : p(a, b) < p_e},      out_ties[e] = #{(a, b) in NE : p(a, b) == p_e}.
 * Every p is cge_link_prob's value and the comparisons are made on those values (the Gram formula only filters, on both sides,
 * with bounds that cost survivors and never correctness), so the counts are a function of the inputs alone: not of the grid, the
 * CU count, the parts or the order of the atomics.
 * `part` of `nparts` (0 <= part < nparts; nparts = 1: everything): the call visits the positions part, part + nparts, ... of the
 * walk of the 128 x 128 pair tiles.  The per-edge counts of the parts add up to the whole exactly; a part without tiles returns
 * zeros; *n_neg is the whole graph's in every part.  (A caller spreads the work over several calls or, by hand, several GPUs.)
 * summary = {W, L, Tq} = {sum w_e, sum w_e less_e, sum w_e ties_e} with the resident edge weights, accumulated on the host in the
 * list's order in long double and rounded once.  The exact local score -- the reference's test is the strict pos > neg, so ties
 * count against -- is 1 - L / (W n_neg); the usual AUC is (L + Tq / 2) / (W n_neg) (sums of ALL parts).  n_neg = 0: the sums are
 * returned, the quotients are the caller's business.
 * CGE_E_ARG, before any device work: no link model; a NULL n_neg or summary; nparts < 1 or part outside 0 .. nparts - 1; under
 * collectives or sharding.  CGE_E_OOM with the bytes named when the scratch (56 bytes per edge) does not fit.  A non-finite
 * embedding is unspecified, as for cge_link_topk.  DESIGN.md section 4.15.
 * Stats: "link_auc_survivors" = pairs of the last call evaluated exactly, "link_auc_tiles", "link_auc_proven" = pairs the filter
 * settled alone.                                                                                                                  */
int cge_link_auc(cge_ctx *ctx, int part, int nparts, int64_t *out_less /* m, may be NULL */, int64_t *out_ties /* m, may be NULL */,
                 double *out_p /* m, may be NULL */, int64_t *n_neg, double summary[3]);
/* The moments of the resident model over EVERY pair, for the resident vertex communities: the global counterpart of cge_link_auc.
 * p(i, j) is the model's probability (cge_link_prob's definition) and q = min(p, 1) what cge_link_sample draws with.
 *   deg_out[i] = sum_{j != i} p(i, j),  deg_in[j] = sum_{i != j} p(i, j)  (undirected: one vector; either pointer or both).
 *   Bins: L = C (C + 1) / 2 undirected in cge_idx(C, min, max) order, L = C * C directed at (comm[i] - 1) * C + comm[j] -- the
 *   layout of the sweep's vect_B / vect_C (src/divergence.jl:55-62, :337-344, :532-537).  C = the largest resident community,
 *   returned in *n_comm.  B[bin] = sum p over the unordered pairs i < j (directed: ordered pairs i != j) whose communities fall in
 *   the bin; V[bin] = sum q (1 - q) over the same pairs, the variance of a draw's edge count there; a bin no pair falls in is 0.
 *   Cobs = the sweep's vect_C of the resident edge list on the vertex communities, by the sweep's own pass.
 * diag = 1 adds the self pairs, as the reference's exact-mode loops do (j in i:no_vertices, :153-158, :229-233): p(i, i) =
 * f_out[i] f_in[i] once to deg_out[i] (directed: and once to deg_in[i]), once to B of bin (c_i, c_i), q (1 - q) of it to V.  On a
 * model left by an exact-mode cge_link_fit(CGE_LINK_BEST_GLOBAL), B with diag = 1 is the sweep's vect_B at the reported alpha.
 * Accuracy: these are sums, NOT defined bit for bit against cge_link_prob.  A pair far enough from coincidence and from the
 * diameter takes its distance from the Gram value of the centred rows; every other pair goes through cge_link_prob's arithmetic.
 * An output that sums the pair set S is within  c sum_S f_out[i] f_in[j]  of the real-number sum, c below 1e-8 for every alpha
 * >= 0.25 and d <= 512 (DESIGN.md section 4.16 derives it) -- an ABSOLUTE bound per pair: a bin of far-apart communities has a
 * tiny sum and the same tolerance.  The outputs ARE a function of the inputs alone: not of the CU count, the grid or the order in
 * which workgroups finish (fixed work items, fixed-order sums, no floating-point atomics).
 * CGE_E_ARG, before any device work: no link model; no resident communities; a NULL n_comm; diag other than 0 / 1; under
 * collectives or sharding.  Every output NULL but n_comm: returns C, no device work.  CGE_E_OOM with the bytes named when the
 * scratch -- 8 dpad ldn + 16 wb 128 items + 64 slots + 16 L + 32 n bytes, section 4.16 -- does not fit.
 * Stats: "link_moments_exact" = pairs evaluated by cge_link_prob's arithmetic, "link_moments_fast" = pairs evaluated from the Gram
 * value (the two add up to the pairs), "link_moments_saturated" = pairs with p > 1 (informational), "link_moments_tiles".        */
int cge_link_moments(cge_ctx *ctx, int diag, double *deg_out /* n, may be NULL */, double *deg_in /* n, may be NULL */,
                     double *B /* L, may be NULL */, double *V /* L, may be NULL */, double *Cobs /* L, may be NULL */,
                     int64_t *n_comm);
/* Expected and observed triangles and wedges, per vertex: how much of the graph's clustering the fitted model explains, without
 * drawing a graph.  Undirected models only.
 * Model side.  q(i, j) = min(p(i, j), 1) is what cge_link_sample draws with, q(i, i) = 0, Q the symmetric matrix of the q (every
 * entry cge_link_prob's value to the bit, clamped).  The edges of a draw are independent, so
 *     tri_exp[i] = 1/2 sum_j Q_ij (Q Q)_ij   (expected triangles through i),
 *     wed_exp[i] = sum_{j < k} Q_ij Q_ik      (expected wedges centred at i).
 * Q is materialised (8 ld^2 bytes, ld = n padded to an odd number of 128-tiles) and Q o (Q Q) is row-summed tile by tile on the
 * fp64 matrix cores; the wedges are summed pair by pair, not as (s1^2 - s2) / 2, which cancels.  Every summand is a product of
 * non-negative doubles, so each output is within
 *     (n + 8) 2^-52 exact  +  n^2 2^-1073
 * of the exact sum over Q's entries (the floor: products that underflow; DESIGN.md section 4.17 derives both).  The outputs are a
 * function of the inputs alone: not of the CU count, the grid or the order in which workgroups finish (fixed work items,
 * fixed-order sums, no floating-point atomics).
 * Graph side.  The resident edge list read as a simple undirected graph -- distinct neighbours, either orientation, repeated rows
 * once, self loops dropped:  tri_obs[v] = triangles through v,  wed_obs[v] = k_v (k_v - 1) / 2 with k_v the distinct neighbours
 * other than v.  Exact integers.
 * summary = {sum tri_exp, sum wed_exp, sum tri_obs, sum wed_obs}, taken on the host in vertex order in long double and rounded
 * once.  Transitivity is summary[0] / summary[1] (model) and summary[2] / summary[3] (graph); triangles are a sum / 3.  The library
 * does not divide: a zero wedge sum is the caller's business.
 * With tri_exp and wed_exp both NULL the model half is not run and summary[0], summary[1] are 0 ("link_tri_tiles" = 0); with one of
 * them NULL its kernel is not run and its sum is 0.  Likewise tri_obs / wed_obs: both NULL skips the graph half, else both sums
 * are returned.
 * CGE_E_ARG, before any device work: no link model; a directed model; a NULL summary; under collectives or sharding.  CGE_E_OOM
 * with the bytes named when Q plus the partials (8 * 128 ceil(n / 128)^2 bytes) do not fit in free memory.
 * Stats: "link_tri_tiles" = 128 x 128 tiles of the last call, "link_tri_saturated" = pairs i < j with p > 1,
 * "link_tri_matrix_bytes" = the bytes of Q.                                                                                      */
int cge_link_triangles(cge_ctx *ctx, double *tri_exp /* n, may be NULL */, double *wed_exp /* n, may be NULL */,
                       int64_t *tri_obs /* n, may be NULL */, int64_t *wed_obs /* n, may be NULL */, double summary[4]);

/* ---- small helpers (same arithmetic as the reference helpers, host side) -------------------- */
int64_t cge_idx(int64_t n, int64_t i, int64_t j);                                   /* src/auxilary.jl:57-59 */
int cge_js(cge_ctx *ctx, const double *vC, const double *vB, int64_t len, const uint8_t *vI, int internal,
           double *out);                                                            /* src/auxilary.jl:34-52 (device) */

/* ---- kernel-level entry points (device work units; used by the parity tests and the bench) -- */
/* per-edge scatter (src/landmarks.jl:433-451 + src/divergence.jl:59-63) on the resident edge list,
 * rows [e0,e1): wedges_out (N x N doubles, [a-1 + (b-1)*N], a<=b when !directed) and vect_C
 * (packed p(C) when !directed, C*C when directed) are HOST outputs (may be NULL).                */
int cge_edge_scatter(cge_ctx *ctx, const int64_t *v_to_l, int64_t N, int64_t C, int directed, int64_t e0,
                     int64_t e1, double *wedges_out, double *vect_C_out);
/* point-set diameter `hi` = maximum(full_graph_D) (src/divergence.jl:104-113) of the resident
 * embedding.  Shard `part` of `nparts` visits its share of the pair tiles (nparts = 1: all);
 * returns the largest distance of the shard's pairs in dist()'s own arithmetic (src/auxilary.jl:14-20;
 * every pair within the Gram formula's rounding bound of the tiles' arg-max is evaluated that way),
 * so the max over shards has the bits of the reference's `hi` whatever the data.  arg_i < arg_j
 * (1-based): a pair attaining it, the smallest (i, j) among ties -- (1, 2) when all rows are equal;
 * a shard without pairs answers 0.  A NaN or Inf anywhere in the embedding: hi = NaN (what
 * extrema() returns in the reference), arg_i = arg_j = 1.                                        */
int cge_max_pair_dist(cge_ctx *ctx, int part, int nparts, double *hi, int64_t *arg_i, int64_t *arg_j);

/* ---- options / statistics --------------------------------------------------------------------- */
/* "diameter": 0 = auto (exact landmark-pair pruning, brute-force MFMA kernel when pruning is weak),
 *             1 = always brute force, 2 = always pruned.  All three return the same exact value.
 * "diameter_f32": how the point-to-reference maxima that bound the landmark pairs of the pruned diameter are computed.
 *             2 (default) = on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16) with every operand split into two bf16 terms,
 *             1 = by fp32-input MFMA (v_mfma_f32_32x32x2_f32); both as rigorous UPPER bounds (fp64 norms, an error margin
 *             of 1.05 (3 (K + 2) 2^-23 + 3.2 2^-16) resp. 1.01 (K + 3) 2^-24 on the dot products, a non-finite accumulator
 *             counted as +Inf; values beyond 2^+-100 send the pass to fp64; K > 128 takes 1 for 2).  0 = in fp64.  The
 *             surviving pairs are evaluated in fp64 as always, so the diameter keeps its bits in every mode.
 * "landmark_edges": 1 = cge_score also builds the N x N landmark-pair matrix and its positive-entry count, i.e. all that
 *             landmarks() returns (src/landmarks.jl:433-463); 0 (default) = on the first cge_landmarks_fetch /
 *             cge_landmarks_info (an undirected score does not read it).  bench.py sets 1.
 * "shard_ingest": N > 1, set AFTER the collectives (cge_comm_init_rccl / cge_set_collectives) and BEFORE the uploads:
 *             1 = cge_set_graph keeps only this rank's slice [m r / W, m (r+1) / W) of the edge list resident (the scatter
 *             passes run over what a rank holds, the sampler's look-ups are exchanged) and cge_set_embedding uploads n / W
 *             rows per rank and all-gathers them device to device; every rank still passes the WHOLE arrays.  Entry points
 *             that need the whole list on one rank (exact-mode cge_score, cge_louvain, cge_edge_scatter, cge_draw_samples,
 *             caller-drawn samples of cge_wgcl) return CGE_E_ARG on a sharded list.  0 (default): every rank uploads and
 *             keeps everything.  Same results.
 * "fit_max_iterations": a Chung-Lu fit (src/divergence.jl:150-168, :434-467) that has not met `diff <= delta` after this many
 *             iterations returns CGE_E_ASSERT "Chung-Lu fit did not converge" (default 2 000 000).  The reference's loop is
 *             unbounded: on a directed graph without a fixed point within delta (e.g. two landmarks, tests/test_gpu_parity.py::
 *             test_directed_fit_without_a_fixed_point_raises) it never returns -- a documented divergence.
 * "shard_rows": N > 1, set AFTER the collectives and BEFORE cge_set_embedding / cge_set_embedding_device, with the communities
 *             already resident (cge_set_vertex_data first): 1 = the EMBEDDING ROWS ARE SHARDED BY COMMUNITY -- communities by
 *             decreasing size, each to the rank with the fewest rows so far; a rank uploads and keeps the rows of its own
 *             communities only (stat "rows_resident" ~ n / W; every rank still passes the whole array) and runs all splits,
 *             forced and global, of those communities.  What crosses ranks: per runsplit round four words per split group
 *             (status, low size, two values) for the replicated heap; v_to_l once (4 B per vertex); the landmarks' centroids /
 *             weights / d_ii once; the bound matrix of the diameter (all-reduce max), the seed row of its sweep and the rows of
 *             the few candidate landmarks of its exact stage; the rows of the sampled pairs of the local score once per seeded
 *             draw; row hashes for the unique-row clamp.  The clusters handed to the landmark phase must refine the community
 *             vector (CGE_E_ARG otherwise).  Entry points that need every row on one rank (exact-mode cge_score,
 *             cge_max_pair_dist, the brute-force diameter option) return CGE_E_ARG.  A later cge_set_vertex_data with ANOTHER
 *             community vector drops the resident rows (upload the embedding again).  0 (default): every rank holds every
 *             row.  Same landmark ids, diameter bits and score.
 * "fit_persistent": how the Chung-Lu fixed point (src/divergence.jl:150-168, :434-467) is launched.
 *             0 = auto: one persistent launch per alpha (the matrix register-resident, the workgroups exchanging
 *                 partial sums and iterates by polling the data itself) for score graphs of >= 128 vertices that fit
 *                 the register file (N <= ~4900 undirected, ~4000 directed on 256 CUs), else one launch per iteration;
 *             1 = always one launch per iteration; 2 = persistent whenever it fits.  Same iterates and iteration counts in
 *             all modes; sums are grouped differently between the launch-per-iteration and the persistent form (last-bit
 *             differences of the score vector).
 * "fit_fused": 1 (default) = in landmark mode (undirected, >= 256 landmarks) the sweep is relabelled by community and the rest
 *             of an alpha's chain rides on the launch of the persistent fit: (1 - D)^alpha in its prologue from the stored
 *             logarithm (no power matrix is written), the community-pair sums of P = T_i T_j (1 - D_ij)^alpha (vect_B,
 *             src/divergence.jl:226-234) per 64 x 64 tile and the tallies of the sampled pairs (:178-213) in its epilogue.
 *             0 = separate launches on the graph as given.  Same iteration counts; the sums of vect_B are grouped differently
 *             (last-bit differences).
 * "wedges_reduce_scatter": N > 1: 1 = the N x N landmark-pair matrix of landmarks() is reduce-scattered by row blocks
 *             (ncclReduceScatter / the hook's reduce_scatter_f64) instead of all-reduced; its consumers then work on row
 *             blocks and cge_landmarks_fetch of the edge list becomes COLLECTIVE (every rank must call it: the blocks are
 *             all-gathered).  0 (default): all-reduce, every fetch is local.
 * "shard_runsplit": with collectives set (N > 1): 1 (default) = the forced per-community phase of runsplit and the big
 *             batches of its global phase are split over the ranks and gathered by one all-reduce each (hook op 2);
 *             0 = runsplit replicated on every rank; 2 = every batch is split (tests).  Same landmark ids in all modes.
 * "shard_samples": with collectives set (N > 1): 1 (default) = from 10^5 local-score samples on, and with the in-library
 *             RCCL communicator, rank r tallies the samples [S r / W, S (r + 1) / W) of every alpha and the block tallies are
 *             all-reduced (2 x 64 doubles per alpha, on the stream); 2 = always (also through the hook; tests); 0 = never.
 *             The sums are grouped differently from a one-rank run (last-bit differences of elements 5-7).
 * "pow_exp2": 1 (default) = GD = (1 - D)^alpha as exp2(alpha * log2(1 - D)) with log2 computed once per score to ~70
 *             bits (a double and a float per entry; below one ulp, like the library pow); 0 = the library pow per alpha.
 * "exact_relabel": exact mode (v_to_l empty) beyond 8192 vertices: 1 (default) = the score graph is relabelled by community
 *             inside the sweep, so that vect_B's row sums are contiguous pieces of a row; 0 = vertices as given (A/B and
 *             tests; same iteration counts, scores equal up to the rounding of the fit's summation order).
 * "exact_packed": the packed form of an undirected exact sweep: the only O(N^2) device storage is the upper tiles of the current
 *             alpha's GD, made from the embedding rows every alpha (no D, no logarithm; one launch pair per fit iteration).  It
 *             applies to N >= 256 vertices in C >= 2 communities with "exact_relabel" on (the sweep is relabelled by community and
 *             vect_B summed by tiles).  0 (default) = used exactly where the resident matrices would be refused
 *             (N N 8 2.2 > 200e9 bytes), so no sweep that ran before changes; 1 = wherever it applies.  The same iteration
 *             counts; scores equal to the resident form's up to the rounding of vect_B's summation order (bit for bit against
 *             a resident sweep with "fit_persistent" = 1 and "bvec_blocks" = 1).  Directed sweeps are not affected.
 * "exact_packed_directed": the packed form of a DIRECTED exact sweep, under the conditions of "exact_packed": the upper tiles of the
 *             current alpha's GD serve the fit (one launch pair per iteration, every tile read once for Sin and Sout of both its
 *             blocks; never a persistent fit), vect_B (a stored tile gives its own partials and its mirror tile's) and the tallies
 *             (ordered pairs); no D, no row-major GD, no logarithm.  0 (default) = never: a directed sweep beyond the resident
 *             limit is refused (CGE_E_OOM), as before; 1 = exactly where the resident matrices would be refused, so no sweep
 *             that ran before changes (cge_cli.py and cge_compare.py set this); 2 = wherever the form applies.  The same
 *             iteration counts; scores equal to the resident form's up to the rounding of the sums' order.  No effect on
 *             undirected sweeps, on landmark mode or on the landmark-mode members of cge_score_batch.
 * "bvec_blocks": 1 = sweeps from 256 vertices on relabel the score graph by community and sum vect_B by 64 x 64 tiles (one read of
 *             GD); 0 (default) = row bins + row sums + fold below 8192 vertices (beyond that the sweep is relabelled and uses the
 *             tiles anyway).  Same results up to the rounding of the summation order; measured no faster at the headline.
 * "ecg_group": cge_ecg runs its members in lock-step groups (one set of launches, one segmented sort and one read-back per round
 *             for the whole group; a member that has stopped is masked out): 0 (default) = as many as half the free memory holds
 *             with group x adjacency entries < 2^31, up to the built-in bound; g = 1 .. 64 = at most g (1: one member at a
 *             time).  The results do not depend on it.  */
int cge_set_option(cge_ctx *ctx, const char *key, int64_t value);
/* "landmarks" (N of the last run, no side effects), "diameter_path" (1 brute / 2 pruned), "diameter_candidate_pairs", "diameter_candidate_tiles", "diameter_refs" (reference points) of the last run;
 * "collective_calls" / "collective_bytes" = all-reduces issued by the in-library RCCL path since cge_create;
 * "diameter_bits" = the bit pattern of the last `hi` (reinterpret the int64 as a double);
 * "fit_batched_launches" / "fit_batched_alphas" = multi-problem fit launches of the last cge_score_batch and the member-alphas they fitted;
 * "exact_packed" = 1 when the last sweep ran in the packed form (options "exact_packed", "exact_packed_directed"), "exact_matrix_bytes" = the bytes of O(N^2)
 * device storage the last exact sweep required (packed: the tiles + the fit's partial vectors, two sets when directed; resident: D + GD + the logarithm it
 * used + the partial vectors of a launch-per-iteration fit);
 * "fit_persistent_alphas" = alphas of the last sweep fitted by a persistent launch, "fit_persistent_fallbacks" = persistent fits abandoned since the context was created, "fit_iterations" = Chung-Lu
 * iterations of the last sweep (all alphas); "landmark_batches" / "landmark_batch_rows" / "landmark_splits" =
 * device batches of the last runsplit, the rows they covered, the groups whose split was computed (those of one or two rows, which need no
 * device batch, included); "landmark_pops" = groups the replay popped (both phases), "landmark_splits_failed" = computed splits that
 * failed, whether or not the group was ever popped (the error is raised only when it is), "landmark_take_rounded" = rounds of the global
 * phase whose batch the 512 rule of 64 < d <= 128 cut down; "cut_tie_tasks" = groups of the size / diameter rules
 * of the last runsplit that held a row exactly ON the cut (settled by the reference's sequential rule; read from the device: synchronises);
 * "edges_resident" / "edges_total" (option shard_ingest), "rows_resident" / "rows_total" (option shard_rows: the embedding rows this
 * rank holds -- about n / W -- and n), "embedding_words_resident" (doubles of the resident row matrix)   */
int cge_get_stat(cge_ctx *ctx, const char *key, int64_t *value);

/* ---- text tables (the step right before the path: `readdlm` at src/auxilary.jl:80-168) -------------------------
 * Parallel reader of a whitespace-delimited numeric table (edge list, community file, embedding): the file is
 * mapped, cut at line boundaries into one piece per thread and parsed with exactly-rounded conversions.  Blank lines
 * are skipped; a first line whose field count differs from the second line's is taken as a header (node2vec's
 * "n d") and skipped, as the reference's retry with skipstart = 1 does (:151-156).  Needs no GPU and no context.
 * n_threads <= 0: one per hardware thread (at most 32).  `err` (optional) receives the message of a failure.
 * open: map the file, find the shape (one pass that counts lines).  parse: convert straight into the caller's matrix,
 * row-major or column-major (Julia's Matrix{Float64}), `out` = rows*cols doubles; no intermediate copy is held, so
 * a table of B bytes of text costs rows*cols*8 bytes of memory and nothing else.                                    */
int cge_text_table_open(const char *path, int n_threads, int64_t *rows, int64_t *cols, int *header_skipped, void **handle,
                        char *err, int64_t err_len);
int cge_text_table_parse(void *handle, double *out, int column_major, char *err, int64_t err_len);
void cge_text_table_close(void *handle);

/* ---- profiling ------------------------------------------------------------------------------ */
/* When enabled, every launch of the named kernels is bracketed by hipEvents on the ctx stream.   */
int cge_profile_enable(cge_ctx *ctx, int on);
int cge_profile_reset(cge_ctx *ctx);
/* restrict the timers to the comma-separated names (NULL or "": every timer); fewer event pairs on the stream        */
int cge_profile_select(cge_ctx *ctx, const char *names);
/* name: "edge_scatter", "max_pair_dist", "fit_symv", ...; returns launches and total milliseconds */
int cge_profile_get(cge_ctx *ctx, const char *name, int64_t *launches, double *total_ms);
int cge_profile_names(cge_ctx *ctx, char *buf, int64_t buf_len); /* comma-separated */
/* wall-clock phase timers of the last cge_score call: "landmarks","aggregate","scatter","dist",
 * "diameter","sweep","samples" (milliseconds, host clock around stream-synchronised phases); after cge_score_batch the
 * last member's, and "batch_sweep" = the shared sweeps of all launch groups ("sweep_setup": a member's set-up of one) */
int cge_phase_ms(cge_ctx *ctx, const char *phase, double *ms);
int cge_phase_names(cge_ctx *ctx, char *buf, int64_t buf_len); /* comma-separated, incl. the lm_* sub-phases */

#ifdef __cplusplus
}
#endif
#endif /* CGE_HIP_H */
