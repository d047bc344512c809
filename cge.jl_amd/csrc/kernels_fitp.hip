// kernels_fitp.hip -- the Chung-Lu fixed points of wGCL / wGCL_directed (src/divergence.jl:150-168, :434-467) as ONE
// persistent launch per alpha: the upper triangle of GD = (1 - D)^alpha lives in REGISTERS for the whole fit.
//
// Why: one iteration streams 8*N*(N+1)/2 algorithmic bytes (64 MB at N = 4000) for 2 flops per byte, a thousand
// times per score.  As one launch per iteration that is ~27 us (the matrix from the Infinity Cache plus a launch
// boundary); here the matrix is read once per alpha and an iteration costs a few KB of exchange between workgroups.
//
// Layout.  The matrix is cut into 64 x 64 tiles; tile (I, J), I <= J, belongs to one wave (tile t -> wave t mod 4G,
// slot t / 4G; G workgroups of 4 waves, at most TPW slots per wave).  Inside a tile lane l = 8*rq + cq holds the
// 8 x 8 block rows 8*rq.., columns 8*cq.. (64 doubles).  One pass over the block gives both products of the
// symmetric pair: p = (T_i*T_j)*g_ij is added to the row sum of i and to the column sum of j (the reference's own
// product, src/divergence.jl:155-158).  The 8 partial rows / columns of a lane are combined across the 8 lanes that
// share rq / cq by a transposing butterfly (4 + 2 + 1 exchanges), which leaves one finished row (column) per lane.
//
// An iteration:  A) every wave: tile products -> partial vectors P[block][other block][64];
//                B) workgroup sb (one 16-row quarter of a block): S_i = sum of the block's Nt partial vectors in a
//                   fixed order, T_i += eps*T_i*(w_i/S_i - 1), f = max|w_i - S_i| (:160-166);
//                C) `while f > delta`, decided by every workgroup from the same maxima.
// Two kernels share this scheme, fit_flow_kernel (undirected) and fit_flow_dir_kernel (directed): THE DATA IS ITS OWN SIGNAL --
// a slot that has not been delivered holds a sentinel and consumers poll the values they need (the header of fit_flow_kernel
// has the re-arming argument).  Every value that crosses workgroups is stored and loaded with agent-scope relaxed atomics
// (sc1: write-through stores, L1-bypassing loads).  Every spin is bounded: on a timeout the launch sets `fail`, every
// workgroup leaves, and the host falls back to one launch per iteration (fit_symtile_kernel + fit_symreduce_kernel below,
// which is also what score graphs beyond the register file use).  All sums have a fixed order: a run is bitwise
// reproducible.  (Rounds 1-4 carried two more forms -- two XCD-hierarchical grid barriers per iteration, 15 us, and per-block
// dependency counters, 10.7 us against 6.1 -- as options 3 / 4 of "fit_persistent"; removed in round 5.)
#include "common.hpp"
#include "pow_parts.hpp"

namespace {

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ double ld_sc1(const double *p) { return __hip_atomic_load(p, RLX_AGENT); }
typedef double dbl2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_sc1(double *p, double v) { __hip_atomic_store(p, v, RLX_AGENT); }
// the same with a wave-uniform base and a 32-bit element index (the buffers of these kernels are far below 4 GB): the
// address is base (scalar registers) + one 32-bit vector offset, so an index that is invariant over the iterations costs
// one vector register to keep instead of two -- fit_flow_kernel runs at the 256-register limit
__device__ __forceinline__ double ld_sc1_at(const double *base, unsigned idx) {
    return ld_sc1(reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + (idx << 3)));
}
__device__ __forceinline__ void st_sc1_at(double *base, unsigned idx, double v) {
    st_sc1(reinterpret_cast<double *>(reinterpret_cast<char *>(base) + (idx << 3)), v);
}

// combine v[0..8) across the 8 lanes that differ in lane bits SH, SH+1, SH+2: afterwards the lane whose three bits
// spell q holds sum_lanes v[q].  Additions are pairwise in a fixed tree.
template <int SH>
__device__ __forceinline__ double transpose_reduce8(const double (&v)[8], int lane) {
    double w4[4], w2[2];
    const bool h2 = (lane >> (SH + 2)) & 1, h1 = (lane >> (SH + 1)) & 1, h0 = (lane >> SH) & 1;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double keep = h2 ? v[q + 4] : v[q], send = h2 ? v[q] : v[q + 4];
        w4[q] = keep + __shfl_xor(send, 4 << SH);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double keep = h1 ? w4[q + 2] : w4[q], send = h1 ? w4[q] : w4[q + 2];
        w2[q] = keep + __shfl_xor(send, 2 << SH);
    }
    const double keep = h0 ? w2[1] : w2[0], send = h0 ? w2[0] : w2[1];
    return keep + __shfl_xor(send, 1 << SH);
}

// ---- the fit with the data as its own signal ------------------------------------------------------------------------
// No counters, no grid barrier: a slot that has not
// been delivered yet holds SENTINEL (a NaN payload that arithmetic never produces), and a consumer polls the values it
// needs until none of them is the sentinel.  A hand-off is then one write-through store and one L1-bypassing load --
// the producer neither drains its stores nor signals, the consumer needs no barrier between a poll and its loads.
// Slots are re-armed by their consumer, off the critical path:
//   T      ring of 4 vectors; T_{k+1} goes to ring[(k+1)&3].  The reducer of a quarter block arms ring[(k+3)&3] (it
//          held T_{k-1}, whose readers have all delivered P_k) while it publishes T_{k+1}; tiles poll that slot for
//          T_{k+3} only after they consumed T_{k+2}, which the same wave stored after an `s_waitcnt vmcnt(0)` that
//          covers the arming store.  T_0 is read from the caller's vector, the result is written to `Tout`.
//   P      two buffers by the parity of k; the reducer arms the entries it has just read, and the tile that rewrites
//          them two iterations later has by then consumed a T_{k+2} stored after the arming stores were drained.
//   f      three buffers (k mod 3): f_k is stored with T_{k+1}, read by every reducer in iteration k+1, armed again by
//          its writer in iteration k+2 -- one iteration before the next value lands there.
// Everything is armed by a fill before the launch.  `done` / `fail` are looked at every 64 polls; a poll never sees a stale
// value, only the sentinel or the value it waits for.
#define FLOW_SENTINEL_WORD 0x7FF8DEADu
#define FLOW_SENTINEL 0x7FF8DEAD7FF8DEADull
__device__ __forceinline__ bool armed(double v) { return (unsigned long long)__double_as_longlong(v) == FLOW_SENTINEL; }
// fit_flow_kernel: a converged reducer stores this where T_{k+1} would go, so the tile waves of workgroups WITHOUT a quarter
// block (G > 4 Nt), which poll that slot, leave at once instead of at their next look at `done` (every 64 polls)
#define FLOW_FINISHED 0x7FF8D0D07FF8D0D0ull
__device__ __forceinline__ bool finished_mark(double v) { return (unsigned long long)__double_as_longlong(v) == FLOW_FINISHED; }
__device__ __forceinline__ double sentinel() { return __longlong_as_double((long long)FLOW_SENTINEL); }
// every 64th unsuccessful poll: 1 = the fit is over, 2 = abandoned (wave-uniform)
// (`done` / `fail` are armed with the sentinel word like everything else of these kernels' buffers: they are SET when they
// hold 1 -- testing them against zero, as rounds 1-2 did, made every wait of more than 64 polls end the fit as "converged")
__device__ __forceinline__ int flow_check(unsigned &spins, unsigned *fail, unsigned *done, long long deadline) {
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & 63u) != 0) return 0;
    if (__hip_atomic_load(done, RLX_AGENT) == 1u) return 1;
    if (wall_clock64() > deadline || __hip_atomic_load(fail, RLX_AGENT) == 1u) {
        __hip_atomic_store(fail, 1u, RLX_AGENT);
        return 2;
    }
    return 0;
}
// max over a row of 16 lanes / over the wave, by DPP (no LDS crossbar); every lane gets the result
template <int CTRL>
__device__ __forceinline__ double dpp_mov64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double row16_max(double v) {
    v = fmax(v, dpp_mov64<0xB1>(v));  // quad_perm [1,0,3,2]
    v = fmax(v, dpp_mov64<0x4E>(v));  // quad_perm [2,3,0,1]
    v = fmax(v, dpp_mov64<0x141>(v)); // row_half_mirror
    v = fmax(v, dpp_mov64<0x140>(v)); // row_mirror
    return v;
}
__device__ __forceinline__ double readlane64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const int hi = __builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_max(double v) {
    v = row16_max(v);
    return fmax(fmax(readlane64(v, 0), readlane64(v, 16)), fmax(readlane64(v, 32), readlane64(v, 48)));
}
// NW waves per workgroup.  With 8 waves of one tile each (two waves per SIMD, 256 registers apiece) the whole tile sits in
// architectural VGPRs and the two waves of a SIMD hide each other's latencies; with 4 waves of two tiles half of the
// matrix lives in accumulation registers and is copied back before use.  The quarter blocks are always reduced by the
// first 256 threads, with the additions of fit_dataflow_kernel in the same order.
#define FLOW_RLD 66 // row stride (doubles) of the transposing-reduction scratch: 16-byte accesses of 8 lanes hit 8 banks groups
// ---- what rides on the fit's launch (round 5): the rest of the alpha's chain, src/divergence.jl:146, :170-176, :178-213, :226-234 ----
// FUSED = true (landmark mode, sweep relabelled by community; wgcl_host.cpp decides):
//   prologue  g = 2^(alpha * log2(1 - D)) from the stored logarithm (pow_parts.hpp: exp2_matrix_upper_kernel's own function and
//             bits) -- the power matrix is never written;
//   epilogue  when the fit has converged the tile and (from the ring) the final T are at hand: the products
//             P_ij = (T_i T_j) g_ij are summed per (row community, column community) rectangle of the tile in the fixed order
//             of bvec_tile_kernel (kernels_fit.hip) -> `partial`, which bvec_bins_kernel folds into vect_B; and the first
//             CGE_PARTIAL_BLOCKS workgroups tally the local score's sampled pairs exactly as auc_landmark_kernel's blocks do.
// Neither launch re-reads the matrix: bvec_rows / bvec_zsum / bvec_fold / exp2_matrix_upper / auc_landmark and one read +
// one write of GD per alpha are gone from the chain.
#define FLOW_NP 32 // pieces (runs of one community inside an 8-column chunk) per 64-column block at most: LDS per wave FLOW_NP x 66 doubles
struct FlowFused { // by value: what the prologue needs, and where the epilogue finds the rest (device memory: loaded after the loop,
                   // so that none of it is held in registers across it -- the loop runs at the register limit)
    const double *Lh; const float *Ll; double alpha; // log2(1 - D) in two parts (k_pow_prepare)
    const cge_fit_fused *epi;                        // device copy of the sweep's table for this sample set
    int want;                                        // bit 0: vect_B's tile partials, bit 1: the local score's tallies
};
// the sum of the first 256 threads' values, block_sum_256's additions (kernels_fit.hip); every thread of the workgroup calls it
__device__ __forceinline__ double flow_sum_256(double v, double *sh, int tid) {
    if (tid < 256) sh[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
template <int TPW, int NW, bool FUSED, int NSB> // NSB: quarter blocks a workgroup may have to reduce (1 when 4*Nt <= G)
__global__ __launch_bounds__(64 * NW) void fit_flow_kernel(const double *__restrict__ GD, i64 N, int Nt, const double *T0,
                                                            double *Tout, i64 Tld, const double *__restrict__ w, double eps,
                                                            double delta, int max_iters, double *ring, double *P, double *fq,
                                                            unsigned *sync, int *flags, long long timeout_ticks, int test_naps,
                                                            const FlowFused fz) {
#define FLOW_WG blockIdx.x
#define FLOW_G gridDim.x
#include "fit_flow_body.inc"
#undef FLOW_WG
#undef FLOW_G
}

// ---- several fused fits in one launch (cge_score_batch) ----------------------------------------------------------------------
// The grid is the concatenation of the problems' grids: workgroup x belongs to problem p, the last whose wg0 is
// <= x, and is its workgroup x - wg0.  Every problem keeps the geometry (G, NW) and the arithmetic of its own fit_flow_kernel<1, NW, true, 1> launch and
// has hand-off slots, flags and epilogue tables of its own, so its iterates, iteration count and epilogue are those of that
// launch.  The host keeps the sum of the G within the CU count (one workgroup per CU, as for one problem): every workgroup of
// every problem is resident, and no problem waits for another.
template <int NW>
__global__ __launch_bounds__(64 * NW) void fit_flow_multi_kernel(const cge_flow_multi tab, double eps, double delta, int max_iters,
                                                                  long long timeout_ticks, int test_naps) {
    constexpr int TPW = 1, NSB = 1;
    constexpr bool FUSED = true;
    int p = 0; // (uniform: the table is a kernel argument)
    for (int i = 1; i < tab.n; i++)
        if ((int)blockIdx.x >= tab.p[i].wg0) p = i;
    const cge_flow_problem &q = tab.p[p];
    const double *__restrict__ GD = nullptr;
    const i64 N = q.N, Tld = q.Tld;
    const int Nt = q.Nt;
    const double *T0 = q.T0, *__restrict__ w = q.w;
    double *Tout = q.Tout, *ring = q.ring, *P = q.P, *fq = q.fq;
    unsigned *sync = q.sync;
    int *flags = q.flags;
    const FlowFused fz = {q.Lh, q.Ll, q.alpha, q.epi, q.want};
#define FLOW_WG ((int)blockIdx.x - q.wg0)
#define FLOW_G q.G
#include "fit_flow_body.inc"
#undef FLOW_WG
#undef FLOW_G
}

// ---- one Chung-Lu iteration per launch pair, over the UPPER tiles only --------------------------------------------
// For landmark counts beyond the register file (N > ~4900: config 5 has 12 000, exact mode N = n) the fit is one
// launch (pair) per iteration and bound by the matrix it streams.  fit_step_kernel (kernels_fit.hip) reads whole rows,
// 8 N^2 bytes per iteration; this form reads every 64 x 64 tile on or above the diagonal once and uses it for both
// products of the symmetric pair, exactly as the persistent kernels do with their register-resident tiles: same lane
// layout (lane 8*rq + cq holds the 8 x 8 block), same transposing reductions, partial vectors P[block][other block][64].
// The second kernel adds a block's Nt partial vectors (four interleaved sequential sums, then ((s0+s1)+s2)+s3 -- a fixed
// order for any Nt), updates T and publishes f: an atomic max on the bit pattern of a non-negative double (exact,
// order-free) in fring[k % 3]; the launch of iteration k + 1 starts by reading f_k -- when it is <= delta the fit is over
// (iters = k + 1, the final T is the one iteration k wrote, exactly the reference's `while diff > delta`) and every later
// launch of the batch returns at `*done`; fring[(k+1) % 3] is cleared by iteration k for iteration k + 1.  Traffic per iteration: 4 N^2 (+ N^2 / 4 for the partial vectors) instead of 8 N^2 bytes.
// PACKED: GD is the upper tiles alone (common.hpp: cge_packed_index) -- lane 8 rq + cq finds its 8 x 8 block of tile t through
// cge_tile_slot, zeros outside the matrix included, and does the same FMAs and additions on it.
template <bool PACKED>
__global__ __launch_bounds__(256) void fit_symtile_kernel(const double *__restrict__ GD, const double *__restrict__ T, i64 N,
                                                          int Nt, i64 NT, double delta, int k,
                                                          const unsigned long long *__restrict__ fring,
                                                          const int *__restrict__ done, double *__restrict__ P) {
    if (*done) return;
    if (k > 0) {
        const double fprev = __longlong_as_double((long long)fring[(k - 1) % 3]);
        if (!(fprev > delta)) return; // the fit ended with iteration k - 1 (the reduce kernel records it)
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rq = lane >> 3, cq = lane & 7;
    const i64 t = (i64)blockIdx.x * 4 + wave;
    if (t >= NT) return;
    // tile t of the row-major upper triangle: start(I) = I*Nt - I*(I-1)/2
    const double bb = 2.0 * Nt + 1.0;
    i64 I = (i64)((bb - sqrt(bb * bb - 8.0 * (double)t)) * 0.5);
    if (I < 0) I = 0;
    if (I > Nt - 1) I = Nt - 1;
    while (I + 1 < Nt && (I + 1) * Nt - (I + 1) * I / 2 <= t) I++;
    while (I > 0 && I * Nt - I * (I - 1) / 2 > t) I--;
    const i64 J = I + (t - (I * Nt - I * (I - 1) / 2));
    const i64 r0 = 64 * I + 8 * rq, c0 = 64 * J + 8 * cq;
    double g[8][8];
    if (PACKED) {
        const double *tile = GD + t * CGE_TILE_DOUBLES;
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const dbl2f v = *reinterpret_cast<const dbl2f *>(tile + cge_tile_slot(8 * rq + a, 8 * cq + 2 * b));
                g[a][2 * b] = v.x;
                g[a][2 * b + 1] = v.y;
            }
    } else if ((N & 1) == 0 && r0 + 8 <= N && c0 + 8 <= N) { // the common case: 16-byte loads, no guards
#pragma unroll
        for (int a = 0; a < 8; a++) {
            const dbl2f *row = reinterpret_cast<const dbl2f *>(GD + (r0 + a) * N + c0);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const dbl2f v = row[b];
                g[a][2 * b] = v.x;
                g[a][2 * b + 1] = v.y;
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = 0; b < 8; b++) g[a][b] = (r0 + a < N && c0 + b < N) ? GD[(r0 + a) * N + c0 + b] : 0.0;
    }
    double ti[8], tj[8], pr[8], pc[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        ti[q] = r0 + q < N ? T[r0 + q] : 0.0;
        tj[q] = c0 + q < N ? T[c0 + q] : 0.0;
        pr[q] = 0.0;
        pc[q] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < 8; a++)
#pragma unroll
        for (int b = 0; b < 8; b++) {
            pr[a] = fma(g[a][b], tj[b], pr[a]); // factored: the row's own T_i is applied by the reducer
            pc[b] = fma(g[a][b], ti[a], pc[b]);
        }
    const double rsum = transpose_reduce8<0>(pr, lane); // row 8*rq + cq of the tile
    P[(I * Nt + J) * 64 + lane] = rsum;
    if (I != J) {
        const double csum = transpose_reduce8<3>(pc, lane); // column 8*cq + rq of the tile
        P[(J * Nt + I) * 64 + 8 * cq + rq] = csum;
    }
}
__global__ __launch_bounds__(256) void fit_symreduce_kernel(const double *__restrict__ P, const double *__restrict__ T,
                                                            double *__restrict__ Tout, const double *__restrict__ w, i64 N,
                                                            int Nt, double eps, double delta, int k,
                                                            unsigned long long *__restrict__ fring, int *__restrict__ done,
                                                            int *__restrict__ iters) {
    __shared__ double red[4][64];
    if (*done) return;
    if (k > 0) {
        const double fprev = __longlong_as_double((long long)fring[(k - 1) % 3]);
        if (!(fprev > delta)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { *iters = k; *done = 1; }
            return;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { fring[(k + 1) % 3] = 0ULL; *iters = k + 1; }
    const int r = threadIdx.x & 63, u = threadIdx.x >> 6;
    const i64 b = blockIdx.x;
    const double *Pb = P + b * Nt * 64 + r;
    double acc = 0.0;
    int q = u;
    for (; q + 12 < Nt; q += 16) { // four loads in flight; the additions stay in q order
        const double p0 = Pb[(i64)q * 64], p1 = Pb[(i64)(q + 4) * 64], p2 = Pb[(i64)(q + 8) * 64], p3 = Pb[(i64)(q + 12) * 64];
        acc += p0; acc += p1; acc += p2; acc += p3;
    }
    for (; q < Nt; q += 4) acc += Pb[(i64)q * 64];
    red[u][r] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const i64 row = 64 * b + r;
        double f = 0.0;
        if (row < N) {
            const double ti = T[row], wi = w[row];
            const double S = ti * (((red[0][r] + red[1][r]) + red[2][r]) + red[3][r]); // the tiles summed g * T
            Tout[row] = ti + (eps * ti) * (wi / S - 1.0);
            f = fabs(wi - S);
        }
        f = wave_max(f);
        if (r == 0) {
            const unsigned long long fb = (unsigned long long)__double_as_longlong(f);
            if (fb > __hip_atomic_load(&fring[k % 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&fring[k % 3], fb);
        }
    }
}
// ---- one DIRECTED Chung-Lu iteration per launch pair, over the upper tiles only ---------------------------------------------
// The directed model's matrix is symmetric (GD[idx(n, min, max)], src/divergence.jl:426-432); only Tin / Tout break the symmetry.
// So one read of the upper tile (I, J) -- fit_symtile_kernel's lane layout and loads -- serves four partial vectors: toward Sin
// and Sout of block I from Tout_J and Tin_J and, for I != J, toward Sin and Sout of block J from Tout_I and Tin_I, factored like
// the undirected form (the row's own Tin_i / Tout_i is applied by the reducer).  The diagonal element is counted twice in both
// sums (:439-449; fit_symv_dir_kernel, kernels_fit.hip, documents the rule): one more FMA in the lanes of a diagonal tile that
// hold the diagonal.  Two passes over the register block (rows, then columns), as fit_flow_dir_body.inc makes them, so that the
// block, one pair of T vectors and one pair of accumulators are live at a time.  Pin / Pout: Nt x Nt x 64 doubles each.
// The reducer adds a block's Nt partial vectors in fit_symreduce_kernel's order, moves Tin / Tout of rows with a positive degree
// (the others are copied: the iterates alternate between two buffers, since other workgroups of the iteration still read the
// old one) and publishes f = max |deg - S| in fring[k % 4].  The epsilon rule needs f of the two previous iterations
// (`if f > diff: eps *= 0.99`, :462-465, eps_0 = 0.9, diff_0 = f0 = 1.0): every workgroup of iteration k derives eps_k from
// f_{k-1}, f_{k-2} and eps_{k-1} = ering[(k - 1) % 2], and workgroup 0 leaves eps_k in ering[k % 2].  A ring of FOUR for f: k - 2,
// k - 1 are read, k is written and k + 1 cleared by one launch.  The end is fit_symtile_kernel's: launch k returns when
// f_{k-1} <= delta, the reducer then records iters = k.
template <bool PACKED>
__global__ __launch_bounds__(256) void fit_symtile_dir_kernel(const double *__restrict__ GD, const double *__restrict__ Tin,
                                                              const double *__restrict__ Tout, i64 N, int Nt, i64 NT, double delta,
                                                              int k, const unsigned long long *__restrict__ fring,
                                                              const int *__restrict__ done, double *__restrict__ Pin,
                                                              double *__restrict__ Pout) {
    if (*done) return;
    if (k > 0) {
        const double fprev = __longlong_as_double((long long)fring[(k - 1) & 3]);
        if (!(fprev > delta)) return; // the fit ended with iteration k - 1 (the reduce kernel records it)
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rq = lane >> 3, cq = lane & 7;
    const i64 t = (i64)blockIdx.x * 4 + wave;
    if (t >= NT) return;
    i64 I, J;
    cge_upper_tile_of(t, Nt, I, J);
    const i64 r0 = 64 * I + 8 * rq, c0 = 64 * J + 8 * cq;
    double g[8][8];
    if (PACKED) {
        const double *tile = GD + t * CGE_TILE_DOUBLES;
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const dbl2f v = *reinterpret_cast<const dbl2f *>(tile + cge_tile_slot(8 * rq + a, 8 * cq + 2 * b));
                g[a][2 * b] = v.x;
                g[a][2 * b + 1] = v.y;
            }
    } else if ((N & 1) == 0 && r0 + 8 <= N && c0 + 8 <= N) { // the common case: 16-byte loads, no guards
#pragma unroll
        for (int a = 0; a < 8; a++) {
            const dbl2f *row = reinterpret_cast<const dbl2f *>(GD + (r0 + a) * N + c0);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const dbl2f v = row[b];
                g[a][2 * b] = v.x;
                g[a][2 * b + 1] = v.y;
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = 0; b < 8; b++) g[a][b] = (r0 + a < N && c0 + b < N) ? GD[(r0 + a) * N + c0 + b] : 0.0;
    }
    { // rows of block I: Sin from Tout_J, Sout from Tin_J
        double to[8], ti[8], pin[8], pout[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            to[q] = c0 + q < N ? Tout[c0 + q] : 0.0;
            ti[q] = c0 + q < N ? Tin[c0 + q] : 0.0;
            pin[q] = 0.0;
            pout[q] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = 0; b < 8; b++) {
                pin[a] = fma(g[a][b], to[b], pin[a]);
                pout[a] = fma(g[a][b], ti[b], pout[a]);
            }
        if (I == J && rq == cq) { // the diagonal term once more
#pragma unroll
            for (int a = 0; a < 8; a++) {
                pin[a] = fma(g[a][a], to[a], pin[a]);
                pout[a] = fma(g[a][a], ti[a], pout[a]);
            }
        }
        const double sin_r = transpose_reduce8<0>(pin, lane), sout_r = transpose_reduce8<0>(pout, lane); // row 8*rq + cq
        Pin[(I * Nt + J) * 64 + lane] = sin_r;
        Pout[(I * Nt + J) * 64 + lane] = sout_r;
    }
    if (I != J) { // rows of block J (the tile's columns): Sin from Tout_I, Sout from Tin_I
        double to[8], ti[8], pin[8], pout[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            to[q] = r0 + q < N ? Tout[r0 + q] : 0.0;
            ti[q] = r0 + q < N ? Tin[r0 + q] : 0.0;
            pin[q] = 0.0;
            pout[q] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < 8; a++)
#pragma unroll
            for (int b = 0; b < 8; b++) {
                pin[b] = fma(g[a][b], to[a], pin[b]);
                pout[b] = fma(g[a][b], ti[a], pout[b]);
            }
        const double sin_c = transpose_reduce8<3>(pin, lane), sout_c = transpose_reduce8<3>(pout, lane); // column 8*cq + rq
        Pin[(J * Nt + I) * 64 + 8 * cq + rq] = sin_c;
        Pout[(J * Nt + I) * 64 + 8 * cq + rq] = sout_c;
    }
}
__global__ __launch_bounds__(256) void fit_symreduce_dir_kernel(const double *__restrict__ Pin, const double *__restrict__ Pout,
                                                                const double *__restrict__ Tin, const double *__restrict__ Tout,
                                                                double *__restrict__ Tin_n, double *__restrict__ Tout_n,
                                                                const double *__restrict__ deg_in,
                                                                const double *__restrict__ deg_out, i64 N, int Nt, double eps0,
                                                                double f0, double delta, int k,
                                                                unsigned long long *__restrict__ fring, double *__restrict__ ering,
                                                                int *__restrict__ done, int *__restrict__ iters) {
    __shared__ double red[2][4][64];
    if (*done) return;
    double eps = eps0;
    if (k > 0) {
        const double f1 = __longlong_as_double((long long)fring[(k - 1) & 3]);
        if (!(f1 > delta)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { *iters = k; *done = 1; }
            return;
        }
        const double f2 = k > 1 ? __longlong_as_double((long long)fring[(k - 2) & 3]) : f0;
        const double ep = ering[(k - 1) & 1];
        eps = f1 > f2 ? ep * 0.99 : ep; // :462-464, after iteration k - 1
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { fring[(k + 1) & 3] = 0ULL; ering[k & 1] = eps; *iters = k + 1; }
    const int r = threadIdx.x & 63, u = threadIdx.x >> 6;
    const i64 b = blockIdx.x;
    const double *Pi = Pin + b * Nt * 64 + r, *Po = Pout + b * Nt * 64 + r;
    double ai = 0.0, ao = 0.0;
    int q = u;
    for (; q + 12 < Nt; q += 16) { // four loads of each in flight; the additions stay in q order
        const double p0 = Pi[(i64)q * 64], p1 = Pi[(i64)(q + 4) * 64], p2 = Pi[(i64)(q + 8) * 64], p3 = Pi[(i64)(q + 12) * 64];
        const double o0 = Po[(i64)q * 64], o1 = Po[(i64)(q + 4) * 64], o2 = Po[(i64)(q + 8) * 64], o3 = Po[(i64)(q + 12) * 64];
        ai += p0; ai += p1; ai += p2; ai += p3;
        ao += o0; ao += o1; ao += o2; ao += o3;
    }
    for (; q < Nt; q += 4) { ai += Pi[(i64)q * 64]; ao += Po[(i64)q * 64]; }
    red[0][u][r] = ai;
    red[1][u][r] = ao;
    __syncthreads();
    if (threadIdx.x < 128) { // wave 0: Tin, wave 1: Tout
        const int s = u;
        const i64 row = 64 * b + r;
        double f = 0.0;
        if (row < N) {
            const double ti = (s ? Tout : Tin)[row], di = (s ? deg_out : deg_in)[row];
            double tn = ti;
            if (di > 0) {
                const double S = ti * (((red[s][0][r] + red[s][1][r]) + red[s][2][r]) + red[s][3][r]); // the tiles summed g * T
                tn = ti + (eps * ti) * (di / S - 1.0);
                f = fabs(di - S);
            }
            (s ? Tout_n : Tin_n)[row] = tn;
        }
        f = wave_max(f);
        if (r == 0) {
            const unsigned long long fb = (unsigned long long)__double_as_longlong(f);
            if (fb > __hip_atomic_load(&fring[k & 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&fring[k & 3], fb);
        }
    }
}
// ---- the directed fit with the data as its own signal (the scheme of fit_flow_kernel) -------------------------------------
// Per tile four partial vectors (e1 = (Tin_i*Tout_j)*g feeds Sin_i and Sout_j, e2 = (Tin_j*Tout_i)*g feeds Sout_i and
// Sin_j, the diagonal term twice), computed in two passes over the register block so that a wave of 256 registers holds
// the tile; the same additions in the same order as fit_dataflow_dir_kernel.  T ring: 4 x (Tin, Tout); P: 2 parities x
// (Sin, Sout) x Nt x Nt x 64; f: 3 x 4Nt.  T_0 = T0 (Tin, Tout: Tld doubles each, zero beyond N); on convergence the
// reducers write their rows of the final iterate to Tin_out / Tout_out (N doubles each), otherwise nothing is written.
template <int NW, int NSB> // NSB: quarter blocks a workgroup may have to reduce (1 when 4*Nt <= G)
__global__ __launch_bounds__(64 * NW) void fit_flow_dir_kernel(const double *__restrict__ GD, i64 N, int Nt, const double *T0,
                                                                double *Tin_out, double *Tout_out, i64 Tld,
                                                                const double *__restrict__ deg_in,
                                                                const double *__restrict__ deg_out, double eps0, double f0,
                                                                double delta, int max_iters, double *ring, double *P,
                                                                double *fq, unsigned *sync, int *flags,
                                                                long long timeout_ticks, int test_naps) {
#define FLOW_WG blockIdx.x
#define FLOW_G gridDim.x
#include "fit_flow_dir_body.inc"
#undef FLOW_WG
#undef FLOW_G
}

// ---- several directed fits in one launch (cge_score_batch on a directed graph) -------------------------------------------------
// As fit_flow_multi_kernel: the grid is the concatenation of the problems' grids, workgroup x belongs to problem p, the last whose
// wg0 is <= x, and is its workgroup x - wg0.  Every problem keeps the geometry (G, NW) and the arithmetic of its own
// fit_flow_dir_kernel<NW, 1> launch and has hand-off slots, start vectors and flags of its own, so its iterates, its iteration
// count and "written on success only" are those of that launch.  The host keeps the sum of the G within the CU count (one
// workgroup per CU): every workgroup of every problem is resident, no problem waits for another, and every spin is bounded by
// the per-iteration deadline of the body (flow_check).
template <int NW>
__global__ __launch_bounds__(64 * NW) void fit_flow_dir_multi_kernel(const cge_flow_dir_multi tab, double eps0, double f0, double delta,
                                                                      int max_iters, long long timeout_ticks, int test_naps) {
    constexpr int NSB = 1;
    int p = 0; // (uniform: the table is a kernel argument)
    for (int i = 1; i < tab.n; i++)
        if ((int)blockIdx.x >= tab.p[i].wg0) p = i;
    const cge_flow_dir_problem &q = tab.p[p];
    const double *__restrict__ GD = q.GD;
    const i64 N = q.N, Tld = q.Tld;
    const int Nt = q.Nt;
    const double *T0 = q.T0;
    double *Tin_out = q.Tin, *Tout_out = q.Tout;
    const double *__restrict__ deg_in = q.deg_in, *__restrict__ deg_out = q.deg_out;
    double *ring = q.ring, *P = q.P, *fq = q.fq;
    unsigned *sync = q.sync;
    int *flags = q.flags;
#define FLOW_WG ((int)blockIdx.x - q.wg0)
#define FLOW_G q.G
#include "fit_flow_dir_body.inc"
#undef FLOW_WG
#undef FLOW_G
}

} // namespace

void k_fit_sym_step(cge_ctx *c, const double *GD, const double *Tin, double *Tout, const double *w, i64 N, double eps,
                    double delta, int k, unsigned long long *fring, int *done, int *iters, bool packed) {
    const int Nt = (int)((N + 63) / 64);
    const i64 NT = (i64)Nt * (Nt + 1) / 2;
    c->fp_P.ensure((size_t)Nt * Nt * 64);
    ScopedKernelTimer t(c, "fit_symv");
    if (packed)
        hipLaunchKernelGGL(fit_symtile_kernel<true>, dim3((unsigned)((NT + 3) / 4)), dim3(256), 0, c->stream, GD, Tin, N, Nt, NT, delta,
                           k, fring, done, c->fp_P.p);
    else
        hipLaunchKernelGGL(fit_symtile_kernel<false>, dim3((unsigned)((NT + 3) / 4)), dim3(256), 0, c->stream, GD, Tin, N, Nt, NT, delta, k,
                           fring, done, c->fp_P.p);
    hipLaunchKernelGGL(fit_symreduce_kernel, dim3((unsigned)Nt), dim3(256), 0, c->stream, c->fp_P.p, Tin, Tout, w, N, Nt, eps,
                       delta, k, fring, done, iters);
}

// Iteration k of the directed fit by the tile pair: (Tin, Tout) -> (Tin_n, Tout_n).  fring: 4 words, zeroed before iteration 0;
// ering: 2 doubles.  The partial vectors are the two halves of fp_P (twice the undirected fit's, which takes the first half).
void k_fit_sym_dir_step(cge_ctx *c, const double *GD, const double *Tin, const double *Tout, double *Tin_n, double *Tout_n,
                        const double *deg_in, const double *deg_out, i64 N, double eps0, double f0, double delta, int k,
                        unsigned long long *fring, double *ering, int *done, int *iters, bool packed) {
    const int Nt = (int)((N + 63) / 64);
    const i64 NT = (i64)Nt * (Nt + 1) / 2;
    const size_t half = (size_t)Nt * Nt * 64;
    c->fp_P.ensure(2 * half);
    double *Pin = c->fp_P.p, *Pout = c->fp_P.p + half;
    ScopedKernelTimer t(c, "fit_symv");
    if (packed)
        hipLaunchKernelGGL(fit_symtile_dir_kernel<true>, dim3((unsigned)((NT + 3) / 4)), dim3(256), 0, c->stream, GD, Tin, Tout, N, Nt,
                           NT, delta, k, fring, done, Pin, Pout);
    else
        hipLaunchKernelGGL(fit_symtile_dir_kernel<false>, dim3((unsigned)((NT + 3) / 4)), dim3(256), 0, c->stream, GD, Tin, Tout, N, Nt,
                           NT, delta, k, fring, done, Pin, Pout);
    hipLaunchKernelGGL(fit_symreduce_dir_kernel, dim3((unsigned)Nt), dim3(256), 0, c->stream, Pin, Pout, Tin, Tout, Tin_n, Tout_n,
                       deg_in, deg_out, N, Nt, eps0, f0, delta, k, fring, ering, done, iters);
}

// ---- the host side of the persistent fits: one geometry, one slot layout, one launch path ------------------------------------
// fit_flow_kernel, fit_flow_multi_kernel, fit_flow_dir_kernel and fit_flow_dir_multi_kernel take their launch shape from
// flow_geometry, the place of their hand-off slots from flow_slots / flow_place, and are checked, armed and launched by
// FlowLaunch.  What differs between the four paths is what is left in their wrappers below: the kernel instance, its arguments,
// and the staging of T_0 for the directed fits.
int device_cus(const cge_ctx *c, bool own) {
    if (!own && c->opt_test_cus > 0) return c->opt_test_cus;
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return cus;
}
// One tile per wave: NW = 4 waves per workgroup while they cover the triangle, else 8 (two per SIMD, 256 registers apiece).  Eight
// tiles per CU is what the register file holds: N <= 4032 on 256 CUs.  G workgroups: one per NW tiles and at least one per quarter
// block where the CUs allow.  Refused: more tiles than waves, more than 64 partial vectors per reducer (Nt > 64), more than two
// quarter blocks per workgroup.
bool flow_geometry(i64 N, int cus, FlowGeometry *g) {
    if (N <= 0 || N > 64 * 64 || cus <= 0) return false;
    const int Nt = (int)((N + 63) / 64);
    const i64 NT = (i64)Nt * (Nt + 1) / 2;
    const int NW = NT <= (i64)4 * cus ? 4 : 8;
    const int G = (int)std::min<i64>(cus, std::max<i64>((NT + NW - 1) / NW, (i64)4 * Nt));
    if (NT > (i64)NW * G || 4 * Nt > 2 * G) return false;
    *g = FlowGeometry{Nt, NT, G, NW, 4 * Nt <= G ? 1 : 2};
    return true;
}
bool flow_geometry(const cge_ctx *c, i64 N, FlowGeometry *g) { return flow_geometry(N, device_cus(c), g); }
// (hand_off / hand_off_directed also refuse G > max_G = cus / 2, whichever kind: the undirected predicate, and with it
// cge_batch_pack_test, does not -- an asymmetry kept as it was)
bool flow_batch_member(i64 N, int cus, bool directed, FlowGeometry *g) {
    return N >= 256 && flow_geometry(N, cus, g) && g->fused() && (!directed || g->G <= cus / 2);
}
FlowSlots flow_slots(int Nt, i64 Tld, bool directed) {
    FlowSlots s;
    s.sync = 0;                                 // 32 doubles: the fail / done words, armed with everything else
    s.ring = s.sync + 32;                       // T ring: 4 x T, directed 4 x (Tin, Tout)
    s.fq = s.ring + (directed ? 8 : 4) * Tld;   // f: 3 x 4 Nt
    s.P = s.fq + 3 * 4 * (i64)Nt;               // P: 2 parities (directed: x (Sin, Sout)) x Nt x Nt x 64
    s.doubles = s.P + (directed ? 4 : 2) * (i64)Nt * Nt * 64;
    return s;
}
// the slot pointers of a problem (cge_flow_problem, cge_flow_dir_problem) whose region starts at `base`
template <class Problem>
static void flow_place(Problem &q, double *base, const FlowSlots &s) {
    q.sync = reinterpret_cast<unsigned *>(base + s.sync);
    q.ring = base + s.ring;
    q.fq = base + s.fq;
    q.P = base + s.P;
}
// What every launch of a persistent fit does around its arguments: the occupancy check of the instance, the limits the kernels
// take (iterations, the deadline per iteration, the test naps), the sentinel fill of a slot region, the timed launch.
struct FlowLaunch {
    cge_ctx *c;
    const void *fn;
    int NW, max_iters = 2000000, naps;
    long long ticks; // per iteration (0: the test hook)
    FlowLaunch(cge_ctx *c_, const void *fn_, int NW_)
        : c(c_), fn(fn_), NW(NW_), naps(c_->opt_fit_test_delay), ticks(c_->opt_fit_test_timeout ? 0LL : CGE_FIT_TIMEOUT_TICKS) {}
    static bool fits(const void *fn, int NW) { // a workgroup of the instance gets a CU
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * NW, 0) == hipSuccess && per_cu >= 1) return true;
        (void)hipGetLastError();
        return false;
    }
    void arm(double *region, i64 doubles) const {
        HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)region, (int)FLOW_SENTINEL_WORD, (size_t)(2 * doubles), c->stream));
    }
    void launch(const char *timer, const char *what, int G, void **args) const {
        hipError_t e;
        {
            ScopedKernelTimer tm(c, timer);
            e = hipLaunchKernel(fn, dim3((unsigned)G), dim3(64 * NW), args, 0, c->stream);
        }
        if (e != hipSuccess) CGE_THROW(CGE_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    }
};

// where the hand-off slots of fit_flow_kernel for N vertices live and how they are armed (the buffer is made if need be)
bool k_fit_flow_arm_region(cge_ctx *c, i64 N, i64 Tld, uint4 **ptr, i64 *n16, unsigned *word) {
    FlowGeometry g;
    if (!flow_geometry(c, N, &g) || Tld < (i64)g.Nt * 64) return false;
    const FlowSlots s = flow_slots(g.Nt, Tld, false);
    if (s.doubles % 2) return false; // (16-byte units)
    c->fp_flow.ensure((size_t)s.doubles);
    *ptr = reinterpret_cast<uint4 *>(c->fp_flow.p);
    *n16 = s.doubles / 2;
    *word = FLOW_SENTINEL_WORD;
    return true;
}
bool k_fit_flow_enqueue(cge_ctx *c, const double *GD, i64 N, const double *T0, double *Tout, i64 Tld, const double *w,
                        double eps, double delta, int *dev_flags, const cge_fit_fused *ff, const cge_fit_fused *ff_dev) {
    const bool fused = ff != nullptr;
    FlowFused fz{};
    if (fused) {
        static_assert(CGE_FLOW_NP == FLOW_NP, "piece limit");
        fz.Lh = ff->Lh; fz.Ll = ff->Ll; fz.alpha = ff->alpha;
        fz.epi = ff_dev;
        fz.want = (ff->partial ? 1 : 0) | (ff->auc_part ? 2 : 0);
    }
    FlowGeometry g;
    if (!flow_geometry(c, N, &g) || Tld < (i64)g.Nt * 64) return false;
    if (fused && !g.fused()) return false; // (callers ask flow_fused_applies first)
    const void *fn;
#define FLOW_PICK(F, B) (g.NW == 8 ? (const void *)fit_flow_kernel<1, 8, F, B> : (const void *)fit_flow_kernel<1, 4, F, B>)
    if (fused) fn = FLOW_PICK(true, 1);
    else fn = g.NSB == 1 ? FLOW_PICK(false, 1) : FLOW_PICK(false, 2);
#undef FLOW_PICK
    if (!FlowLaunch::fits(fn, g.NW)) return false;
    FlowLaunch L(c, fn, g.NW);
    const FlowSlots s = flow_slots(g.Nt, Tld, false);
    c->fp_flow.ensure((size_t)s.doubles);
    if (c->flow_armed_words != 2 * s.doubles) // (else: armed by the last launch of the previous alpha's chain, bins_js_kernel)
        L.arm(c->fp_flow.p, s.doubles);
    c->flow_armed_words = 0;
    cge_flow_problem q{};
    flow_place(q, c->fp_flow.p, s);
    void *args[] = {&GD, &N, &g.Nt, &T0, &Tout, &Tld, &w, &eps, &delta, &L.max_iters, &q.ring, &q.P, &q.fq, &q.sync, &dev_flags,
                    &L.ticks, &L.naps, &fz};
    L.launch("fit_persistent", "fit", g.G, args);
    return true;
}

static const void *flow_multi_fn(int NW, bool directed) {
    if (!directed) return NW == 8 ? (const void *)fit_flow_multi_kernel<8> : (const void *)fit_flow_multi_kernel<4>;
    return NW == 8 ? (const void *)fit_flow_dir_multi_kernel<8> : (const void *)fit_flow_dir_multi_kernel<4>;
}
bool k_fit_flow_multi_fits(int NW, bool directed) { return FlowLaunch::fits(flow_multi_fn(NW, directed), NW); }
// What the two shared launches have in common: the count first, every problem's first workgroup wg0 in the concatenated grid,
// the test that the grid is resident (one workgroup per CU), and the problems' slot regions back to back in `flow`, which also
// gets room for `stage` x Tld doubles per problem behind them.  Returns the slots' doubles in all; *grid = the sum of the G.
template <class Tab>
static i64 flow_multi_place(const cge_ctx *c, Tab &tab, bool directed, int stage, DevBuf<double> &flow, int *grid) {
    const char *kind = directed ? "directed " : "";
    if (tab.n < 1 || tab.n > CGE_BATCH_MAX) CGE_THROW(CGE_E_ASSERT, "%sfit batch of %d problems", kind, tab.n);
    const int cus = device_cus(c);
    i64 tot = 0, extra = 0;
    int wg = 0;
    for (int i = 0; i < tab.n; i++) {
        tab.p[i].wg0 = wg;
        wg += tab.p[i].G;
        tot += flow_slots(tab.p[i].Nt, tab.p[i].Tld, directed).doubles;
        extra += stage * tab.p[i].Tld;
    }
    if (wg > cus) CGE_THROW(CGE_E_ASSERT, "%sfit batch of %d problems on %d workgroups does not fit %d CUs", kind, tab.n, wg, cus);
    flow.ensure((size_t)(tot + extra));
    i64 off = 0;
    for (int i = 0; i < tab.n; i++) {
        const FlowSlots s = flow_slots(tab.p[i].Nt, tab.p[i].Tld, directed);
        flow_place(tab.p[i], flow.p + off, s);
        off += s.doubles;
    }
    *grid = wg;
    return tot;
}
void k_fit_flow_multi(cge_ctx *c, cge_flow_multi &tab, int NW, double eps, double delta, DevBuf<double> &flow) {
    int grid = 0;
    const i64 tot = flow_multi_place(c, tab, false, 0, flow, &grid);
    FlowLaunch L(c, flow_multi_fn(NW, false), NW);
    L.arm(flow.p, tot); // every slot armed
    void *args[] = {&tab, &eps, &delta, &L.max_iters, &L.ticks, &L.naps};
    L.launch("fit_batched", "batched fit", grid, args);
}
// `flow`: the problems' slot regions (armed with one fill), then their T_0 (Tin, Tout: Tld doubles each, zero beyond N), staged
// here from the problem's Tin / Tout, which the launch updates on success only
void k_fit_flow_dir_multi(cge_ctx *c, cge_flow_dir_multi &tab, int NW, double eps0, double f0, double delta, DevBuf<double> &flow) {
    int grid = 0;
    const i64 tot = flow_multi_place(c, tab, true, 2, flow, &grid);
    hipStream_t st = c->stream;
    FlowLaunch L(c, flow_multi_fn(NW, true), NW);
    L.arm(flow.p, tot); // every slot armed
    i64 t0tot = 0;
    for (int i = 0; i < tab.n; i++) t0tot += 2 * tab.p[i].Tld;
    HIP_CHECK(hipMemsetAsync(flow.p + tot, 0, sizeof(double) * t0tot, st));
    double *t0 = flow.p + tot;
    for (int i = 0; i < tab.n; i++) {
        cge_flow_dir_problem &q = tab.p[i];
        HIP_CHECK(hipMemcpyAsync(t0, q.Tin, sizeof(double) * q.N, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemcpyAsync(t0 + q.Tld, q.Tout, sizeof(double) * q.N, hipMemcpyDeviceToDevice, st));
        q.T0 = t0;
        t0 += 2 * q.Tld;
    }
    void *args[] = {&tab, &eps0, &f0, &delta, &L.max_iters, &L.ticks, &L.naps};
    L.launch("fit_batched", "batched directed fit", grid, args);
}

// Directed fit of one alpha from Tin / Tout (N doubles each, updated in place on success).  Returns false when the
// persistent path does not apply or was abandoned; Tin / Tout are then untouched.
bool k_fit_persistent_dir(cge_ctx *c, const double *GD, i64 N, double *Tin, double *Tout, const double *deg_in,
                          const double *deg_out, double eps0, double f0, double delta, i64 *iters, int *dev_flags, bool *enqueued_only) {
    if (enqueued_only) *enqueued_only = false;
    FlowGeometry g;
    if (!flow_geometry(c, N, &g)) return false; // (the caller iterates with one launch pair per iteration)
    const void *fn = g.NW == 8 ? (g.NSB == 1 ? (const void *)fit_flow_dir_kernel<8, 1> : (const void *)fit_flow_dir_kernel<8, 2>)
                               : (g.NSB == 1 ? (const void *)fit_flow_dir_kernel<4, 1> : (const void *)fit_flow_dir_kernel<4, 2>);
    if (!FlowLaunch::fits(fn, g.NW)) return false;
    FlowLaunch L(c, fn, g.NW);
    hipStream_t st = c->stream;
    i64 Tld = (i64)g.Nt * 64;
    const FlowSlots s = flow_slots(g.Nt, Tld, true);
    c->fp_Td.ensure((size_t)4 * Tld);
    c->fp_flow.ensure((size_t)s.doubles);
    c->flow_armed_words = 0; // (the undirected fit's slots live in the same buffer)
    c->fp_flags.ensure(4);
    HIP_CHECK(hipMemsetAsync(c->fp_Td.p, 0, sizeof(double) * 2 * Tld, st)); // T_0 = (Tin, Tout), zero beyond N
    HIP_CHECK(hipMemcpyAsync(c->fp_Td.p, Tin, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(c->fp_Td.p + Tld, Tout, sizeof(double) * N, hipMemcpyDeviceToDevice, st));
    L.arm(c->fp_flow.p, s.doubles);
    cge_flow_dir_problem q{};
    flow_place(q, c->fp_flow.p, s);
    q.T0 = c->fp_Td.p;
    q.flags = dev_flags ? dev_flags : c->fp_flags.p;
    void *args[] = {&GD, &N, &g.Nt, &q.T0, &Tin, &Tout, &Tld, &deg_in, &deg_out, &eps0, &f0, &delta, &L.max_iters, &q.ring, &q.P,
                    &q.fq, &q.sync, &q.flags, &L.ticks, &L.naps};
    L.launch("fit_persistent", "directed fit", g.G, args);
    if (dev_flags) { // enqueue only: the caller reads the verdict (flags) behind whatever it queues after the fit
        *enqueued_only = true;
        *iters = 0;
        return true;
    }
    int hf[4];
    HIP_CHECK(hipMemcpyAsync(hf, c->fp_flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (hf[2] || !hf[0]) { // abandoned: Tin / Tout are untouched
        note_fit_fallback(c);
        return false;
    }
    *iters = hf[1];
    return true;
}

