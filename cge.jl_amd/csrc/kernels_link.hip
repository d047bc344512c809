// kernels_link.hip -- the link model's kernels (cge_link_*, link_host.cpp): the per-vertex factors of a fitted model, the model's
// probability of given pairs, per query the k most probable candidates, and the exact rank of given pairs among their query's
// candidates (link_rank_kernel: top-k's tiles and filter stage with thresholds known before the first tile), and draws of the random
// graph the model is (link_sample_kernel: max_pair_kernel's walk of all pair tiles, a filter of its own), and the exact link AUC
// (link_auc_kernel: the same walk, rank's filter, every non-edge placed among the edges' sorted values), and the model's sums over
// every pair (link_moments_kernel, at the end: expected degrees and community bins in fixed-order partials).  gfx950 only.
//
//     p(i, j) = (f_out[i] * f_in[j]) * max(0, 1 - dist(i, j) / hi) ^ alpha
//
// link_p below is the ONE definition of that value: cge_link_prob evaluates it per pair, and the top-k kernel evaluates it for every
// pair its filter lets through, so a reported p is cge_link_prob's to the bit and the ranking is by those values.
//
// Top-k (one more member of the distance-kernel family, next to max_pair_kernel's "running max" and the packed store): a workgroup
// owns one 128-query row tile and one slice of the 128-candidate tiles, runs gram_tile_128 (mfma_tile.hpp) per tile on the centred
// feature-major operands of the diameter (Xc / rnorm; the queries gathered into the same form), and its epilogue FILTERS:
//   * every query row keeps tau_i, the k-th value of its list so far (none while the list is short: everything passes);
//   * a pair can only enter the list when p >= tau_i, and p <= f_out[i] fmax (1 - d / hi)^alpha with fmax the largest f_in of the
//     candidate tile, i.e. when d^2 <= R2_i = (hi (1 - (tau_i / (f_out[i] fmax))^(1 / alpha)))^2 -- taken with margins that cover the
//     roundings of p's own evaluation (link_radius2);
//   * the Gram value g = r_i + r_j - 2 <x_i, x_j> of the centred rows is within (K + 16) 2^-52 (r_i + r_j) of the squared
//     distance (the (K + 8) 2^-52 (r_i + r_j) derived at pcent_kernel in kernels_dist.hip, plus the centring's own rounding and
//     the two additions of the threshold), so the test  g <= R2_i + e (r_i + r_j)  loses no pair that belongs in the list,
//     whatever the rounding did.  Per pair it costs max_pair_kernel's gram_value, one addition and one compare.
// Survivors are marked in a 128 x 128 bit mask in LDS; then each wave takes 32 rows, evaluates a row's survivors exactly from the
// rows in global memory (link_p), drops the query itself and -- when edges are excluded -- the pairs found in the sorted edge keys,
// and merges them into the row's list by rank under the total order (p descending, j ascending).  The lists live in global
// scratch (128 rows x 64 entries x 12 bytes do not fit beside the 73.7 KB of Gram staging twice per CU); after the first tile
// insertions are rare.  A second kernel merges the slices' lists per query under the same order.
#include "mfma_tile.hpp"
#include "link_p.hpp"

#include <rocprim/rocprim.hpp>

#define LK_KMAX 64
#define LK_MAX_SLICES 512 // the merge kernel keeps nsl / 64 <= 8 list heads per lane
#define LK_EXTRA_DOUBLES (128 /* tau */ + 128 /* thr */ + 256 /* mask: 128 x 4 words */ + 64 /* counts: 128 ints */ + 128 /* rq */)
#define LK_LDS_BYTES ((size_t)2 * 2 * MP_BK * MP_LD * sizeof(double) + (size_t)LK_EXTRA_DOUBLES * sizeof(double))
// link_rank_kernel: erow, arow, asure, rq (128 doubles each) and the 128 x 4 words of the mask
#define LR_LDS_BYTES ((size_t)2 * 2 * MP_BK * MP_LD * sizeof(double) + (size_t)(4 * 128 + 256) * sizeof(double))

// (link_dist, link_power, link_p -- the one definition of the value -- and lds_sync: link_p.hpp)

// ---- the factors of a fitted model ------------------------------------------------------------------------------------------------
__global__ void link_expand_kernel(const double *__restrict__ Ta, const double *__restrict__ Tb, const i32 *__restrict__ v2l,
                                   const double *__restrict__ vw, const double *__restrict__ lw, i64 n, double *__restrict__ fo,
                                   double *__restrict__ fi) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    if (!v2l) {
        fo[v] = Ta[v];
        fi[v] = Tb[v];
        return;
    }
    const i64 l = v2l[v];
    fo[v] = (Ta[l] * vw[v]) / lw[l]; // auc_landmark_kernel's ai / aj
    fi[v] = (Tb[l] * vw[v]) / lw[l];
}
void k_link_expand(cge_ctx *c, const double *Ta, const double *Tb, const i32 *v2l, const double *vw, const double *lw, i64 n,
                   double *f_out, double *f_in) {
    hipLaunchKernelGGL(link_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, Ta, Tb, v2l, vw, lw, n, f_out,
                       f_in);
}
__global__ void link_tile_max_kernel(const double *__restrict__ f, i64 n, double *__restrict__ ftile) {
    const i64 j = (i64)blockIdx.x * 128 + threadIdx.x;
    double v = j < n ? f[j] : 0.0;
    v = fmax(v, __shfl_xor(v, 32));
    v = fmax(v, __shfl_xor(v, 16));
    v = fmax(v, __shfl_xor(v, 8));
    v = fmax(v, __shfl_xor(v, 4));
    v = fmax(v, __shfl_xor(v, 2));
    v = fmax(v, __shfl_xor(v, 1));
    __shared__ double s[2];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) ftile[blockIdx.x] = fmax(s[0], s[1]);
}
void k_link_tile_max(cge_ctx *c, const double *f_in, i64 n, i64 ntiles, double *ftile) {
    hipLaunchKernelGGL(link_tile_max_kernel, dim3((unsigned)ntiles), dim3(128), 0, c->stream, f_in, n, ftile);
}

// ---- cge_link_prob ----------------------------------------------------------------------------------------------------------------
template <bool EXP2>
__global__ void link_prob_kernel(const double *__restrict__ Xr, i64 d, const i32 *__restrict__ pi, const i32 *__restrict__ pj, i64 P,
                                 const double *__restrict__ fo, const double *__restrict__ fi, double hi, double alpha,
                                 double *__restrict__ out) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += stride) {
        const i64 i = pi[q], j = pj[q];
        out[q] = link_p<EXP2>(Xr, d, i, j, fo[i], fi[j], hi, alpha);
    }
}
void k_link_prob(cge_ctx *c, const i32 *pi, const i32 *pj, i64 P, double *out) {
    if (P <= 0) return;
    const LinkModel &m = c->link;
    ScopedKernelTimer t(c, "link_prob");
    const dim3 grid(grid_for(P, 128, 256 * 16));
    if (m.pow_form)
        hipLaunchKernelGGL(link_prob_kernel<true>, grid, dim3(128), 0, c->stream, c->Xr.p, c->d, pi, pj, P, m.f.p, m.f.p + m.n, m.hi,
                           m.alpha, out);
    else
        hipLaunchKernelGGL(link_prob_kernel<false>, grid, dim3(128), 0, c->stream, c->Xr.p, c->d, pi, pj, P, m.f.p, m.f.p + m.n, m.hi,
                           m.alpha, out);
}

// ---- the resident edge list as sorted keys ----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long link_key(i64 a, i64 b, int directed) {
    if (!directed && a > b) { const i64 t = a; a = b; b = t; }
    return ((unsigned long long)(unsigned)a << 32) | (unsigned long long)(unsigned)b;
}
__global__ void link_keys_kernel(const i32 *__restrict__ src, const i32 *__restrict__ dst, i64 m, int directed,
                                 unsigned long long *__restrict__ keys) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) keys[e] = link_key(src[e], dst[e], directed);
}
void k_link_keys(cge_ctx *c) {
    LinkModel &m = c->link;
    if (m.keys_ready) return;
    const i64 ne = c->m;
    m.keys_in.ensure((size_t)ne);
    m.keys.ensure((size_t)ne);
    ScopedKernelTimer t(c, "link_keys");
    hipLaunchKernelGGL(link_keys_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c->stream, c->src.p, c->dst.p, ne, m.directed,
                       m.keys_in.p);
    size_t bytes = 0;
    HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, m.keys_in.p, m.keys.p, (size_t)ne, 0u, 64u, c->stream));
    c->sort_tmp.ensure(bytes);
    HIP_CHECK(rocprim::radix_sort_keys(c->sort_tmp.p, bytes, m.keys_in.p, m.keys.p, (size_t)ne, 0u, 64u, c->stream));
    m.nkeys = ne;
    m.keys_ready = true;
}
__device__ __forceinline__ bool link_is_edge(const unsigned long long *__restrict__ keys, i64 nkeys, unsigned long long key) {
    i64 lo = 0, hi = nkeys; // first position with keys[pos] >= key
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < nkeys && keys[lo] == key;
}

// ---- cge_link_topk ----------------------------------------------------------------------------------------------------------------
// what the two tiled queries (top-k, rank) share: the operands of the Gram tiles, the model, the filter's constants, the edge keys
struct LinkTiles {
    const double *Xq, *rq; i64 ldq;   // the queries, centred feature-major (dpad x ldq) and their squared norms
    const double *Xc, *rn; i64 ldn;   // the candidates: every vertex, the same form
    i64 n, Q, dpad;
    int nsl;
    const i32 *qid;                    // the queries' vertex ids (Q)
    const double *Xr; i64 d;           // the rows as dist() reads them
    const double *fo, *fi, *ftile;
    double hi, alpha, einfl, dinfl;
    const unsigned long long *keys; i64 nkeys; int directed; // keys == nullptr: nothing is excluded
    unsigned long long *surv;          // pairs evaluated exactly (a stat)
};
struct LinkTopk : LinkTiles {
    int k;
    double *lp; i32 *lj, *lcnt;        // the lists: [(row tile * nsl + slice) * 128 + row][k], and their lengths
};
// cge_link_rank: the distinct queries' pairs grouped, a query's thresholds descending
struct LinkRank : LinkTiles {
    const i64 *off;                    // [Q + 1]: query q's pairs are off[q] .. off[q + 1] of t
    const double *t;                   // the pairs' own probabilities (cge_link_prob's values)
    unsigned long long *G, *E;         // per pair slot: candidates that first exceed it / that equal its run (at the run's start)
    const double *fib;                 // f_in[c]^(-1 / alpha): the candidate's part of the filter's root
};

// The squared radius beyond which no candidate of a tile can reach tau: den = f_out[i] fmax(tile).  p's own evaluation rounds (two
// products, a power within an ulp or two, the base 1 - d / hi, d itself a K-term sum): the quotient is shrunk by 1e-12, the root by
// 1e-12 (1 + 1 / alpha) -- which also leaves 1 - r an absolute 1e-12 -- and the radius is stretched by dinfl = 1 + (K + 16) 2^-52.
__device__ __forceinline__ double link_radius2(double tau, double den, double hi, double alpha, double dinfl) {
    const double inf = __builtin_huge_val();
    if (!(tau > 0.0)) return inf;  // a short list (tau < 0), or a k-th value of 0: ties at 0 admit every candidate
    if (!(den > 0.0)) return -inf; // every p of this tile is 0 < tau
    double q = (tau / den) * (1.0 - 1e-12);
    if (q > 1.0) q = 1.0;
    double r = pow(q, 1.0 / alpha) * (1.0 - 1e-12 * (1.0 + 1.0 / alpha));
    if (!(r > 0.0)) r = 0.0;
    const double R = hi * (1.0 - r) * dinfl;
    return R * R * (1.0 + 1e-15);
}
// (p, j) before (q, l) in the lists' total order
__device__ __forceinline__ bool link_before(double p, i32 j, double q, i32 l) { return p > q || (p == q && j < l); }

// ---- the filter stage of the tiled queries (top-k and rank): ONE copy ---------------------------------------------------------------
// this tile's thresholds from the rows' tau and the tile's largest f_in, the rows' share of the rounding bound added
__device__ __forceinline__ void link_filter_thresholds(const LinkTiles &A, int tid, i64 i0, i64 J, const double *tau,
                                                       const double *rqs, double *thr) {
    if (tid < 128) {
        const i64 qi = i0 + tid;
        double t = -__builtin_huge_val();
        if (qi < A.Q) t = link_radius2(tau[tid], A.fo[A.qid[qi]] * A.ftile[J], A.hi, A.alpha, A.dinfl) + A.einfl * rqs[tid];
        thr[tid] = t;
    }
}
// the filter: acc[a][b][r] is row i0 + wr*64 + a*16 + lk + 4r, column j0 + wc*64 + b*16 + lr; a pair within its limit sets its bit
// of the 128 x 128 mask.  The limit of a pair is  thr[row] + e r_j  (PERCAND = false: thr is this tile's squared radius of the row,
// its share of the rounding bound added -- link_filter_thresholds), or, with the candidate's own factor in the place of the tile's
// largest (PERCAND = true: link_rank_kernel, whose thresholds never move),
//     (hi (1 - min(1, a_i b_c)) dinfl)^2 (1 + 1e-15) + (erow_i + e r_j),    a_i = thr[row] (link_root_row),  b_c = f_in[c]^(-1 / alpha):
// link_radius2's expression with the root of the quotient taken as a product of a row's and a candidate's root.
// SURE (with PERCAND): the other side of the same bound.  A pair whose Gram value proves p > the row's LARGEST threshold sets its
// bit of mask2 as well: with a+_i = asure[row] (link_root_row_sure),  r+ = a+_i b_c + 1e-12 < 1  and
//     g + e (r_i + r_j) < ((hi / dinfl) (1 - r+))^2 (1 - 1e-14).
// Then the true squared distance is below the right side (g is within e (r_i + r_j) of it), dist()'s K-term sum and the quotient
// by hi stay below hi (1 - r+) and 1 - r+ (the 1 / dinfl, at least 17 u of the quotient where the base is small; where it is not,
// the relative margins of r+ are four orders above u), the base 1 - x is at least r+ - 1e-12 >= a+_i b_c, and a+_i b_c is the
// root of t_max / (f_out f_in) stretched by 1e-12 in the quotient and 2e-12 (1 + 1 / alpha) in the root: the power of the base
// (within two ulp) times the two factors (an ulp each) exceeds t_max by more than 1e-12 of it.
template <bool PERCAND, bool SURE = false>
__device__ __forceinline__ void link_filter_mask(const LinkTiles &A, const d4 (&acc)[4][4], i64 j0, const double *rqs,
                                                 const double *thr, const double *erow, const double *fib, unsigned *mask, int wr,
                                                 int wc, int lr, int lk, const double *asure = nullptr, unsigned *mask2 = nullptr) {
    const double hsure = SURE ? A.hi / A.dinfl : 0.0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int jl = wc * 64 + b * 16 + lr;
        const i64 j = j0 + jl;
        const double rj = A.rn[j]; // rnorm is padded to ldn
        const double ej = A.einfl * rj;
        if (j < A.n) {
            const double bc = PERCAND ? fib[j] : 0.0;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int il = wr * 64 + a * 16 + lk + 4 * r;
                    const double g = gram_value(rqs[il], rj, acc[a][b][r]);
                    double lim;
                    if (PERCAND) {
                        const double R = A.hi * (1.0 - fmin(thr[il] * bc, 1.0)) * A.dinfl;
                        lim = R * R * (1.0 + 1e-15) + (erow[il] + ej);
                    } else {
                        lim = thr[il] + ej;
                    }
                    bool pass = g <= lim;
                    if (SURE) {
                        const double rp = asure[il] * bc + 1e-12;
                        const double Rm = hsure * (1.0 - rp);
                        if (rp < 1.0 && g + (A.einfl * rqs[il] + ej) < Rm * Rm * (1.0 - 1e-14)) {
                            atomicOr(&mask2[il * 4 + (jl >> 5)], 1u << (jl & 31));
                            pass = true;
                        }
                    }
                    if (pass) atomicOr(&mask[il * 4 + (jl >> 5)], 1u << (jl & 31));
                }
        }
    }
}
// The row's part of the root r = (tau / (f_out[i] f_in[c]))^(1 / alpha) = a_i b_c of link_radius2, with its margins: the quotient
// shrunk by 1e-12, the root by 2e-12 (1 + 1 / alpha) -- link_radius2's 1e-12 (1 + 1 / alpha) and as much again for the roundings of
// b_c (a pow, within two ulp) and of the product, five orders of magnitude below it.  -inf: every candidate passes (tau = 0: ties at
// 0 admit everything, whatever the distance); +inf: none does.  A product that underflows only widens the radius.
__device__ __forceinline__ double link_root_row(double tau, double fo, double alpha) {
    const double inf = __builtin_huge_val();
    if (!(tau > 0.0)) return -inf;
    if (!(fo > 0.0)) return inf; // (tau = f_out[i] ... > 0 has f_out[i] > 0)
    const double q = (tau / fo) * (1.0 - 1e-12);
    if (!(q < inf)) return -inf;
    return pow(q, 1.0 / alpha) * (1.0 - 2e-12 * (1.0 + 1.0 / alpha));
}
// the row's part of r+ (link_filter_mask, SURE): the root of t_max / f_out[i] with the margins on the other side; +inf: nothing
// is proven (a largest threshold of 0, a NaN)
__device__ __forceinline__ double link_root_row_sure(double tmax, double fo, double alpha) {
    const double inf = __builtin_huge_val();
    if (!(tmax > 0.0) || !(fo > 0.0)) return inf;
    const double q = (tmax / fo) * (1.0 + 1e-12);
    if (!(q < inf)) return inf;
    return pow(q, 1.0 / alpha) * (1.0 + 2e-12 * (1.0 + 1.0 / alpha));
}
// a row's survivors, two candidates per lane (j0 + lane, j0 + lane + 64): the exact value of those that are admissible -- not the
// query itself, not a resident neighbour when edges are excluded -- and -1 for the rest; returns this lane's count of mask bits.
// SURE: an admissible survivor whose bit of ms is set is not evaluated (the filter has proven it above every threshold): -2.
template <bool EXP2, bool SURE = false>
__device__ __forceinline__ int link_row_survivors(const LinkTiles &A, const uint4 mw, i64 vi, double fo, i64 j0, int lane,
                                                  double (&pc)[2], i32 (&jc)[2], const uint4 ms = uint4{0u, 0u, 0u, 0u}) {
    const unsigned w0 = lane < 32 ? mw.x : mw.y, w1 = lane < 32 ? mw.z : mw.w;
    const unsigned s0 = lane < 32 ? ms.x : ms.y, s1 = lane < 32 ? ms.z : ms.w;
    int nsurv = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const i64 j = j0 + lane + 64 * h;
        bool on = (((h ? w1 : w0) >> (lane & 31)) & 1u) != 0u;
        const bool sure = SURE && (((h ? s1 : s0) >> (lane & 31)) & 1u) != 0u;
        nsurv += on && !sure ? 1 : 0;
        on = on && j != vi;
        if (on && A.keys) on = !link_is_edge(A.keys, A.nkeys, link_key(vi, j, A.directed));
        pc[h] = !on ? -1.0 : sure ? -2.0 : link_p<EXP2>(A.Xr, A.d, vi, j, fo, A.fi[j], A.hi, A.alpha);
        jc[h] = (i32)j;
    }
    return nsurv;
}

template <bool EXP2>
__global__ __launch_bounds__(256, 2) void link_topk_kernel(LinkTopk A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *tau = lds + (size_t)2 * 2 * MP_BK * MP_LD, *thr = tau + 128;
    unsigned *mask = reinterpret_cast<unsigned *>(thr + 128);
    int *cnt = reinterpret_cast<int *>(mask + 512);
    double *rqs = reinterpret_cast<double *>(cnt + 128); // the squared norms of the tile's 128 query rows
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4, c2 = lane * 2;
    const i64 It = blockIdx.x / A.nsl;
    const int sl = (int)(blockIdx.x % A.nsl);
    const i64 i0 = It * MP_BM, nTc = A.ldn / MP_BN, nchunk = A.dpad / MP_BK;
    const int k = A.k;
    const i64 list0 = ((i64)blockIdx.x * 128) * k; // this workgroup's 128 lists
    if (tid < 128) {
        tau[tid] = -1.0;
        cnt[tid] = 0;
        rqs[tid] = A.rq[i0 + tid]; // rq is padded to ldq
    }
    for (int q = tid; q < 512; q += 256) mask[q] = 0u;
    // per wave: the scratch of a row's merge, in the Gram staging (free between two tiles): 192 values and ids
    unsigned long long wsurv = 0;
    double *mp = lds + (size_t)wave * 320;
    i32 *mj = reinterpret_cast<i32 *>(mp + 192);
    lds_sync();
    for (i64 J = sl; J < nTc; J += A.nsl) {
        const i64 j0 = J * MP_BN;
        d4 acc[4][4];
        gram_tile_128(A.Xq + (i64)wave * A.ldq + i0 + c2, A.Xc + (i64)wave * A.ldn + j0 + c2, A.ldq, A.ldn, nchunk, lds, acc, wave,
                      c2, wr, wc, lr, lk);
        link_filter_thresholds(A, tid, i0, J, tau, rqs, thr);
        lds_sync();
        link_filter_mask<false>(A, acc, j0, rqs, thr, nullptr, nullptr, mask, wr, wc, lr, lk);
        lds_sync();
        // ---- the survivors, row by row: wave w takes the rows w, w + 4, ...
        for (int rr = 0; rr < 32; rr++) {
            const int il = wave + 4 * rr;
            const uint4 mw = *reinterpret_cast<const uint4 *>(mask + il * 4);
            if ((mw.x | mw.y | mw.z | mw.w) == 0u) continue; // (wave-uniform)
            const i64 vi = A.qid[i0 + il]; // (a row beyond Q has an empty mask: its threshold is -inf)
            const double fo = A.fo[vi];
            double pc[2];
            i32 jc[2];
            const int nsurv = link_row_survivors<EXP2>(A, mw, vi, fo, j0, lane, pc, jc);
            if (lane < 4) mask[il * 4 + lane] = 0u;
            int tot = nsurv; // the survivors of this row, a stat (added up per wave, one atomic at the end)
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) tot += __shfl_xor(tot, s);
            wsurv += (unsigned long long)tot;
            // a full list whose k-th value every survivor of the row stays below (the filter's bound is the tile's largest f_in,
            // most candidates' own is smaller) is left as it is: no merge
            const double tcur = tau[il]; // (-1 while the list is short: every admissible survivor enters)
            if (!__any((pc[0] >= 0.0 && pc[0] >= tcur) || (pc[1] >= 0.0 && pc[1] >= tcur))) continue;
            const int have = cnt[il];
            double *lp = A.lp + list0 + (i64)il * k;
            i32 *lj = A.lj + list0 + (i64)il * k;
            const double pl = lane < have ? lp[lane] : -1.0;
            const i32 jl_ = lane < have ? lj[lane] : 0;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // (the previous row's readers of the scratch are this wave: in order)
            mp[lane] = pl; mj[lane] = jl_;
            mp[64 + lane] = pc[0]; mj[64 + lane] = jc[0];
            mp[128 + lane] = pc[1]; mj[128 + lane] = jc[1];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            // rank of each of this lane's three entries among the valid ones (p >= 0; a NaN never enters)
            int rk[3] = {0, 0, 0}, valid = 0;
            const double ep[3] = {pl, pc[0], pc[1]};
            const i32 ej3[3] = {jl_, jc[0], jc[1]};
            for (int e = 0; e < 192; e++) {
                const double q = mp[e];
                const i32 l = mj[e];
                if (q >= 0.0) {
                    valid++;
#pragma unroll
                    for (int u = 0; u < 3; u++) rk[u] += link_before(q, l, ep[u], ej3[u]) ? 1 : 0;
                }
            }
            const int now = valid < k ? valid : k;
#pragma unroll
            for (int u = 0; u < 3; u++)
                if (ep[u] >= 0.0 && rk[u] < k) {
                    lp[rk[u]] = ep[u];
                    lj[rk[u]] = ej3[u];
                    if (now == k && rk[u] == k - 1) tau[il] = ep[u];
                }
            if (lane == 0) cnt[il] = now;
            __threadfence_block(); // the list entries are read back by other lanes of this wave at the row's next merge
        }
        // (the next tile's staging is written behind gram_tile_128's first barrier: every wave is done with its scratch by then)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // tau, the counts and the cleared masks have landed before that barrier
    }
    lds_sync();
    if (tid < 128) A.lcnt[(i64)blockIdx.x * 128 + tid] = cnt[tid];
    if (lane == 0 && wsurv) atomicAdd(A.surv, wsurv);
}

// the slices' lists of a query merged under the same order: one wave per query, lane l holds the heads of slices l, l + 64, ...
__global__ __launch_bounds__(64) void link_merge_kernel(const double *__restrict__ lp, const i32 *__restrict__ lj,
                                                       const i32 *__restrict__ lcnt, i64 Q, int k, int nsl, i64 *__restrict__ out_j,
                                                       double *__restrict__ out_p, i64 *__restrict__ out_cnt) {
    const i64 q = blockIdx.x;
    const int lane = threadIdx.x;
    const i64 It = q / 128, il = q % 128;
    int head[LK_MAX_SLICES / 64], len[LK_MAX_SLICES / 64];
#pragma unroll
    for (int u = 0; u < LK_MAX_SLICES / 64; u++) {
        const int s = lane + 64 * u;
        head[u] = 0;
        len[u] = s < nsl ? lcnt[(It * nsl + s) * 128 + il] : 0;
    }
    int t = 0;
    for (; t < k; t++) {
        double bp = -1.0;
        i32 bj = 0x7fffffff;
        int bu = -1;
#pragma unroll
        for (int u = 0; u < LK_MAX_SLICES / 64; u++)
            if (head[u] < len[u]) {
                const i64 at = ((It * nsl + lane + 64 * u) * 128 + il) * (i64)k + head[u];
                const double p = lp[at];
                const i32 j = lj[at];
                if (bu < 0 || link_before(p, j, bp, bj)) { bp = p; bj = j; bu = u; }
            }
        double wp = bp;
        i32 wj = bj;
        int wany = bu >= 0 ? 1 : 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const double op = __shfl_xor(wp, s);
            const i32 oj = __shfl_xor(wj, s);
            const int oany = __shfl_xor(wany, s);
            if (oany && (!wany || link_before(op, oj, wp, wj))) { wp = op; wj = oj; wany = 1; }
        }
        if (!wany) break;
        if (bu >= 0 && bj == wj) { // (a candidate sits in one slice only: its id names the winner)
#pragma unroll
            for (int u = 0; u < LK_MAX_SLICES / 64; u++)
                if (u == bu) head[u]++;
        }
        if (lane == 0) {
            out_j[q * k + t] = (i64)wj + 1;
            out_p[q * k + t] = wp;
        }
    }
    if (lane == 0) out_cnt[q] = t;
    for (int u = t + lane; u < k; u += 64) {
        out_j[q * k + u] = 0;
        out_p[q * k + u] = 0.0;
    }
}

void k_link_topk(cge_ctx *c, const i32 *qid, i64 Q, int k, bool exclude, i64 *out_j, double *out_p, i64 *out_cnt) {
    LinkModel &m = c->link;
    const i64 nQt = (Q + 127) / 128, ldq = nQt * 128, nTc = c->ldn / 128;
    // enough slices of the candidate tiles to fill the CUs twice over when the queries are few
    i64 nsl = (2 * (i64)device_cus(c) + nQt - 1) / nQt;
    nsl = std::max<i64>(1, std::min<i64>(std::min<i64>(nsl, nTc), LK_MAX_SLICES));
    const i64 nwg = nQt * nsl;
    if (nwg > 0x7fffffffLL) CGE_THROW(CGE_E_ARG, "link_topk: %lld workgroups exceed a launch", (long long)nwg);
    m.Xq.ensure((size_t)ldq * c->dpad);
    m.rq.ensure((size_t)ldq);
    m.lp.ensure((size_t)nwg * 128 * k);
    m.lj.ensure((size_t)nwg * 128 * k);
    m.lcnt.ensure((size_t)nwg * 128);
    m.surv.ensure(1);
    k_gather_centre_fm(c, c->Xr.p, qid, c->gmean.p, m.Xq.p, m.rq.p, Q, c->d, ldq, c->dpad);
    LinkTopk A{};
    A.Xq = m.Xq.p; A.rq = m.rq.p; A.ldq = ldq;
    A.Xc = c->Xc.p; A.rn = c->rnorm.p; A.ldn = c->ldn;
    A.n = c->n; A.Q = Q; A.dpad = c->dpad;
    A.k = k; A.nsl = (int)nsl;
    A.qid = qid;
    A.Xr = c->Xr.p; A.d = c->d;
    A.fo = m.f.p; A.fi = m.f.p + m.n; A.ftile = m.ftile.p;
    A.hi = m.hi; A.alpha = m.alpha;
    A.einfl = (double)(c->dpad + 16) * 2.220446049250313e-16; // (K + 16) 2^-52
    A.dinfl = 1.0 + A.einfl;
    A.keys = exclude ? m.keys.p : nullptr; A.nkeys = exclude ? m.nkeys : 0; A.directed = m.directed;
    A.lp = m.lp.p; A.lj = m.lj.p; A.lcnt = m.lcnt.p;
    A.surv = m.surv.p;
    {
        ScopedKernelTimer t(c, "link_topk");
        if (m.pow_form) {
            cge_allow_lds((const void *)link_topk_kernel<true>, LK_LDS_BYTES);
            hipLaunchKernelGGL(link_topk_kernel<true>, dim3((unsigned)nwg), dim3(256), LK_LDS_BYTES, c->stream, A);
        } else {
            cge_allow_lds((const void *)link_topk_kernel<false>, LK_LDS_BYTES);
            hipLaunchKernelGGL(link_topk_kernel<false>, dim3((unsigned)nwg), dim3(256), LK_LDS_BYTES, c->stream, A);
        }
    }
    ScopedKernelTimer t(c, "link_merge");
    hipLaunchKernelGGL(link_merge_kernel, dim3((unsigned)Q), dim3(64), 0, c->stream, m.lp.p, m.lj.p, m.lcnt.p, Q, k, (int)nsl, out_j,
                       out_p, out_cnt);
}

// ---- cge_link_rank ----------------------------------------------------------------------------------------------------------------
// Per vertex the number of distinct excluded neighbours other than itself, from the sorted keys: the first of every run of equal
// keys counts, a self loop does not; undirected keys are (min, max) and count for both ends, directed ones for the source.
__global__ void link_excl_kernel(const unsigned long long *__restrict__ keys, i64 nkeys, int directed, i32 *__restrict__ excl) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < nkeys; e += stride) {
        const unsigned long long key = keys[e];
        if (e > 0 && keys[e - 1] == key) continue;
        const i64 a = (i64)(key >> 32), b = (i64)(key & 0xffffffffull);
        if (a == b) continue;
        atomicAdd(&excl[a], 1);
        if (!directed) atomicAdd(&excl[b], 1);
    }
}
// the candidate's part of the rank filter's root: f_in[c]^(-1 / alpha) (a zero factor: +inf, no radius at all)
__global__ void link_fib_kernel(const double *__restrict__ fi, i64 n, double alpha, double *__restrict__ fib) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) fib[v] = pow(fi[v], -1.0 / alpha);
}
void k_link_fib(cge_ctx *c) {
    LinkModel &m = c->link;
    if (m.fib_ready) return;
    m.fib.ensure((size_t)m.n);
    hipLaunchKernelGGL(link_fib_kernel, dim3((unsigned)((m.n + 255) / 256)), dim3(256), 0, c->stream, m.f.p + m.n, m.n, m.alpha, m.fib.p);
    m.fib_ready = true;
}
void k_link_excl(cge_ctx *c) {
    LinkModel &m = c->link;
    if (m.excl_ready) return;
    k_link_keys(c);
    m.excl.ensure((size_t)m.n);
    HIP_CHECK(hipMemsetAsync(m.excl.p, 0, sizeof(i32) * (size_t)m.n, c->stream));
    ScopedKernelTimer t(c, "link_excl");
    hipLaunchKernelGGL(link_excl_kernel, dim3(grid_for(m.nkeys, 256)), dim3(256), 0, c->stream, m.keys.p, m.nkeys, m.directed,
                       m.excl.p);
    m.excl_ready = true;
}

// The rank of given pairs among their query's candidates.  Top-k's geometry and top-k's filter, but a row's tau is known before
// the first tile -- the smallest probability among the query's own pairs -- so there is no list, no warm-up and no merge.  A
// survivor (p_c, c) of row i is placed by binary search in the row's descending thresholds t[off_i ..]: with s0 the first slot
// whose threshold is below p_c, every pair from s0 on has c above it (one add into G[off_i + s0]; an inclusive prefix sum over
// the row gives `greater`), and the run of slots equal to p_c, if any, has c as a tie (one add at the run's first slot of E).
// Integer atomics: the counts do not depend on the grid, the slicing or the order.
template <bool EXP2>
__global__ __launch_bounds__(256, 2) void link_rank_kernel(LinkRank A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *erow = lds + (size_t)2 * 2 * MP_BK * MP_LD, *arow = erow + 128, *asure = arow + 128, *rqs = asure + 128;
    unsigned *mask = reinterpret_cast<unsigned *>(rqs + 128);
    unsigned *mask2 = reinterpret_cast<unsigned *>(lds); // the proven pairs of a tile: in the Gram staging, free between two tiles
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4, c2 = lane * 2;
    const i64 It = blockIdx.x / A.nsl;
    const int sl = (int)(blockIdx.x % A.nsl);
    const i64 i0 = It * MP_BM, nTc = A.ldn / MP_BN, nchunk = A.dpad / MP_BK;
    if (tid < 128) { // a row's tau is the smallest of its thresholds, the last of its group, and the first is the largest: both are
        const i64 qi = i0 + tid; // fixed for the launch, and so are their roots
        const double rq = A.rq[i0 + tid]; // rq is padded to ldq
        const double inf = __builtin_huge_val();
        double ar = inf, as = inf;
        if (qi < A.Q) {
            const double fo = A.fo[A.qid[qi]];
            ar = link_root_row(A.t[A.off[qi + 1] - 1], fo, A.alpha);
            as = link_root_row_sure(A.t[A.off[qi]], fo, A.alpha);
        }
        rqs[tid] = rq;
        arow[tid] = ar;
        asure[tid] = as;
        erow[tid] = qi < A.Q ? A.einfl * rq : -inf; // (a row beyond Q passes nothing, whatever its Gram value)
    }
    for (int q = tid; q < 512; q += 256) mask[q] = 0u;
    unsigned long long wsurv = 0;
    lds_sync();
    for (i64 J = sl; J < nTc; J += A.nsl) {
        const i64 j0 = J * MP_BN;
        d4 acc[4][4];
        gram_tile_128(A.Xq + (i64)wave * A.ldq + i0 + c2, A.Xc + (i64)wave * A.ldn + j0 + c2, A.ldq, A.ldn, nchunk, lds, acc, wave,
                      c2, wr, wc, lr, lk);
        // (gram_tile_128 ends behind a barrier: every wave is done with the staging)
        for (int q = tid; q < 512; q += 256) mask2[q] = 0u;
        lds_sync();
        link_filter_mask<true, true>(A, acc, j0, rqs, arow, erow, A.fib, mask, wr, wc, lr, lk, asure, mask2);
        lds_sync();
        // ---- the survivors, row by row: wave w takes the rows w, w + 4, ...
        for (int rr = 0; rr < 32; rr++) {
            const int il = wave + 4 * rr;
            const uint4 mw = *reinterpret_cast<const uint4 *>(mask + il * 4);
            if ((mw.x | mw.y | mw.z | mw.w) == 0u) continue; // (wave-uniform)
            const uint4 ms = *reinterpret_cast<const uint4 *>(mask2 + il * 4);
            const i64 vi = A.qid[i0 + il]; // (a row beyond Q has an empty mask: its erow is -inf, its asure +inf)
            const double fo = A.fo[vi];
            double pc[2];
            i32 jc[2];
            const int nsurv = link_row_survivors<EXP2, true>(A, mw, vi, fo, j0, lane, pc, jc, ms);
            if (lane < 4) mask[il * 4 + lane] = 0u;
            int tot = nsurv, above = (pc[0] == -2.0 ? 1 : 0) + (pc[1] == -2.0 ? 1 : 0); // evaluated exactly; proven above every threshold
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                tot += __shfl_xor(tot, s);
                above += __shfl_xor(above, s);
            }
            wsurv += (unsigned long long)tot;
            const i64 o0 = A.off[i0 + il], np = A.off[i0 + il + 1] - o0;
            if (lane == 0 && above) atomicAdd(A.G + o0, (unsigned long long)above); // above the first slot: greater for every pair
            const double *t = A.t + o0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const double p = pc[h];
                if (!(p >= 0.0)) continue; // not admissible (-1), or a NaN
                i64 lo = 0, hi = np; // the first slot with t <= p: the slots before it are above p
                while (lo < hi) {
                    const i64 mid = (lo + hi) >> 1;
                    if (t[mid] > p) lo = mid + 1;
                    else hi = mid;
                }
                const i64 eq0 = lo;
                hi = np; // the first slot with t < p, from there on
                while (lo < hi) {
                    const i64 mid = (lo + hi) >> 1;
                    if (t[mid] >= p) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < np) atomicAdd(A.G + o0 + lo, 1ull);
                if (eq0 < lo) atomicAdd(A.E + o0 + eq0, 1ull);
            }
        }
        // (the next tile's staging is written behind gram_tile_128's first barrier: every wave has read its rows of mask2 by then)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the cleared masks have landed before that barrier
    }
    if (lane == 0 && wsurv) atomicAdd(A.surv, wsurv);
}

// One wave per distinct query: the inclusive prefix sum of its G (64 slots a round, the carry passed on) is `greater` of every
// pair; `ties` is the E of the pair's run minus the pair's own j where that is a candidate; `cand` from the excluded-neighbour
// counts.  Written through the permutation to the caller's order.
__global__ __launch_bounds__(64) void link_rank_final_kernel(const i32 *__restrict__ uq, const i64 *__restrict__ off,
                                                            const double *__restrict__ t, const i32 *__restrict__ gj,
                                                            const i64 *__restrict__ perm, const unsigned long long *__restrict__ G,
                                                            const unsigned long long *__restrict__ E,
                                                            const unsigned long long *__restrict__ keys, i64 nkeys, int directed,
                                                            const i32 *__restrict__ excl, i64 n, i64 *__restrict__ out_greater,
                                                            i64 *__restrict__ out_ties, i64 *__restrict__ out_cand) {
    const i64 q = blockIdx.x;
    const int lane = threadIdx.x;
    const i64 vi = uq[q], o0 = off[q], np = off[q + 1] - o0;
    const i64 nexcl = keys ? (i64)excl[vi] : 0;
    unsigned long long carry = 0;
    for (i64 s0 = 0; s0 < np; s0 += 64) {
        const i64 s = s0 + lane;
        unsigned long long g = s < np ? G[o0 + s] : 0ull;
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) {
            const unsigned long long up = __shfl_up(g, w);
            if (lane >= w) g += up;
        }
        g += carry;
        carry = __shfl(g, 63);
        if (s < np) {
            const double ts = t[o0 + s];
            i64 lo = 0, hi = s; // the first slot of the run equal to ts (descending thresholds: the first with t <= ts)
            while (lo < hi) {
                const i64 mid = (lo + hi) >> 1;
                if (t[o0 + mid] > ts) lo = mid + 1;
                else hi = mid;
            }
            const i64 j = gj[o0 + s];
            const bool j_excl = keys && link_is_edge(keys, nkeys, link_key(vi, j, directed));
            const i64 at = perm[o0 + s];
            out_greater[at] = (i64)g;
            out_ties[at] = (i64)E[o0 + lo] - (j_excl ? 0 : 1);
            out_cand[at] = n - 1 - nexcl - (j_excl ? 0 : 1);
        }
    }
}

void k_link_rank(cge_ctx *c, const i32 *uq, const i64 *off, i64 Qu, const double *t, unsigned long long *G,
                 unsigned long long *E, bool exclude) {
    LinkModel &m = c->link;
    const i64 nQt = (Qu + 127) / 128, ldq = nQt * 128, nTc = c->ldn / 128;
    // enough slices of the candidate tiles to fill the CUs twice over when the queries are few (nothing is merged per slice:
    // no other limit than the tiles)
    i64 nsl = (2 * (i64)device_cus(c) + nQt - 1) / nQt;
    nsl = std::max<i64>(1, std::min<i64>(nsl, nTc));
    const i64 nwg = nQt * nsl;
    if (nwg > 0x7fffffffLL) CGE_THROW(CGE_E_ARG, "link_rank: %lld workgroups exceed a launch", (long long)nwg);
    m.Xq.ensure((size_t)ldq * c->dpad);
    m.rq.ensure((size_t)ldq);
    k_link_fib(c);
    k_gather_centre_fm(c, c->Xr.p, uq, c->gmean.p, m.Xq.p, m.rq.p, Qu, c->d, ldq, c->dpad);
    LinkRank A{};
    A.Xq = m.Xq.p; A.rq = m.rq.p; A.ldq = ldq;
    A.Xc = c->Xc.p; A.rn = c->rnorm.p; A.ldn = c->ldn;
    A.n = c->n; A.Q = Qu; A.dpad = c->dpad;
    A.nsl = (int)nsl;
    A.qid = uq;
    A.Xr = c->Xr.p; A.d = c->d;
    A.fo = m.f.p; A.fi = m.f.p + m.n; A.ftile = m.ftile.p;
    A.hi = m.hi; A.alpha = m.alpha;
    A.einfl = (double)(c->dpad + 16) * 2.220446049250313e-16; // (K + 16) 2^-52
    A.dinfl = 1.0 + A.einfl;
    A.keys = exclude ? m.keys.p : nullptr; A.nkeys = exclude ? m.nkeys : 0; A.directed = m.directed;
    A.surv = m.surv.p;
    A.off = off; A.t = t; A.G = G; A.E = E;
    A.fib = m.fib.p;
    ScopedKernelTimer tm(c, "link_rank");
    if (m.pow_form) {
        cge_allow_lds((const void *)link_rank_kernel<true>, LR_LDS_BYTES);
        hipLaunchKernelGGL(link_rank_kernel<true>, dim3((unsigned)nwg), dim3(256), LR_LDS_BYTES, c->stream, A);
    } else {
        cge_allow_lds((const void *)link_rank_kernel<false>, LR_LDS_BYTES);
        hipLaunchKernelGGL(link_rank_kernel<false>, dim3((unsigned)nwg), dim3(256), LR_LDS_BYTES, c->stream, A);
    }
}
void k_link_rank_final(cge_ctx *c, const i32 *uq, const i64 *off, i64 Qu, const double *t, const i32 *gj, const i64 *perm,
                       const unsigned long long *G, const unsigned long long *E, bool exclude, i64 *out_greater, i64 *out_ties,
                       i64 *out_cand) {
    LinkModel &m = c->link;
    if (Qu > 0x7fffffffLL) CGE_THROW(CGE_E_ARG, "link_rank: %lld queries exceed a launch", (long long)Qu);
    ScopedKernelTimer tm(c, "link_rank_final");
    hipLaunchKernelGGL(link_rank_final_kernel, dim3((unsigned)Qu), dim3(64), 0, c->stream, uq, off, t, gj, perm, G, E,
                       exclude ? m.keys.p : nullptr, exclude ? m.nkeys : 0, m.directed, exclude ? m.excl.p : nullptr, m.n, out_greater,
                       out_ties, out_cand);
}

// ---- cge_link_sample --------------------------------------------------------------------------------------------------------------
// One draw of the random graph the model IS: every pair is an edge when u(i, j) < p(i, j), u the counter stream's uniform of the
// pair (which = 5), p link_p's value.  max_pair_kernel's geometry -- a strided walk of the upper 128 x 128 tiles in super-block
// order (directed: of all tiles) on the centred feature-major operands -- and top-k's two stages: the tile's epilogue FILTERS, a
// wave per row evaluates the survivors exactly and appends the edges' keys (a << 32 | b) behind one atomic per row.  The keys are
// sorted afterwards, so the result does not depend on the grid or on the order of the appends.
//
// The filter rejects a pair only when it has proven u >= p.  u is a multiple of 2^-53 (or the hook's value); with
// ff = fl(f_out[i] f_in[j]) and the power pw of the computed base b = fl(1 - x), x = fl(dist / hi), p = fl(ff pw):
//   stage 1   pw <= 1 (b <= 1, either form of the power), so p <= ff: a pair with u >= ff (1 + 1e-12) is no edge.  In a fitted
//             model of a sparse graph ff is of the order of the edge density: whole waves stop here.
//   stage 2   in the log2 domain, with hardware f32 root and logarithm.  glo = max(0, g - e (r_i + r_j)) is a lower bound of the
//             squared distance (e = (K + 16) 2^-52, the bound top-k filters by), q = glo / hi^2 in fp64 (two roundings),
//                 xf = sqrt_f32((float)q) (1 - 2^-20):  the conversion (2^-24 of q, 2^-25 of the root), the root (an ulp, 2^-23) and
//             the product (2^-24) stay below 2^-22, the rest of the 2^-20 is beyond dist()'s own (K / 2 + 3) 2^-53 (a K-term sum,
//             a root, a quotient), so xf <= x whatever the rounding did;
//                 B = fl32(fl32(max(0, 1 - xf)) + 2^-22) >= max(0, b):  the two f32 additions round by at most 2^-25 + 2^-24;
//             B > 0 also where the base is clamped (hi below the diameter: p = 0 <= any bound) and where q overflows f32 (x > 1);
//                 p <= ff B^alpha (1 + 6 u):  the power within two ulp, two products;
//                 log2 p <= lf_out[i] + lf_in[j] + alpha log2 B + 2^-49, the tables log2 f in fp64 (below 2^-42 each, as are the
//             three fp64 operations of the sum).  log2_f32 is within an ulp of a result below 64 in magnitude (B >= 2^-22,
//             u >= 2^-53): 2^-18, taken as 2^-16, once for u and alpha times for B; (float)u is at most u (1 + 2^-24), 2^-23 in
//             the logarithm.  Together below (1 + alpha) 2^-16 + 2^-22;
//                 slack = (1 + alpha) 2^-14
//             is four times that.  A pair is rejected when log2_f32((float)u) >= lf_out[i] + lf_in[j] + alpha log2_f32(B) + slack.
//             The slack widens the bound on p by (1 + alpha) 4.2e-5 of it, and the f32 steps by about alpha 1.4e-6 / b: survivors,
//             never a wrong answer.  A zero factor: ff = 0, stage 1 rejects (u >= 0 = p).  u = 0, or anything below 2^-100 (the
//             stream gives no such value but 0; the hook might): stage 2 is not asked, the f32 logarithm of such a value is not
//             covered by the above.  p >= 1: u < 1 <= p <= ff, and log2 u < 0 < the right side.  A NaN on the right side passes.
struct LinkSample {
    const double *Xc, *rn; i64 ldn, n, dpad; // the centred feature-major operand and the squared norms
    const double *Xr; i64 d;                 // the rows as dist() reads them
    const double *fo, *fi, *lfo, *lfi;       // the factors and their log2
    double hi, alpha, einfl, inv_hi2, slack;
    int directed;
    unsigned long long h2;                   // the counter stream after its rounds of seed and stream
    const double *U; int ulay;               // the hook: u(a, b) = U[a n + b] (ulay = 0: U[min n + max])
    unsigned long long *keys; i64 cap;       // the edges' keys; beyond cap they are counted and not stored
    unsigned long long *cnt;                 // [0] edges, [1] pairs evaluated exactly
};
#define LS_LDS_BYTES ((size_t)2 * 2 * MP_BK * MP_LD * sizeof(double) + (size_t)(4 * 128 + 256) * sizeof(double))

// the last two rounds of cge_ctr_rand(seed, stream, a, b, 5), from the row's key (the first three: link_row_key)
__device__ __forceinline__ unsigned long long link_row_key(unsigned long long h2, i64 a) {
    return cge_sm64(h2 ^ ((unsigned long long)a * 0x2545f4914f6cdd1dULL + 2));
}
template <bool UMAT>
__device__ __forceinline__ double link_uniform(const LinkSample &A, unsigned long long rowkey, i64 a, i64 b) {
    if (UMAT) return A.U[(A.ulay || a < b) ? a * A.n + b : b * A.n + a];
    const unsigned long long h = cge_sm64(rowkey ^ ((unsigned long long)b * 0x9e6c63d0676a9a99ULL + 3));
    return (double)(cge_sm64(h ^ 9ULL) >> 11) * 0x1p-53;
}

template <bool EXP2, bool UMAT>
__global__ __launch_bounds__(256, 2) void link_sample_kernel(LinkSample A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *rqs = lds + (size_t)2 * 2 * MP_BK * MP_LD, *fos = rqs + 128, *lfs = fos + 128;
    unsigned long long *rkey = reinterpret_cast<unsigned long long *>(lfs + 128);
    unsigned *mask = reinterpret_cast<unsigned *>(rkey + 128);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4, c2 = lane * 2;
    const i64 nT = A.ldn / MP_BM, nS = (nT + MP_SB - 1) / MP_SB, nchunk = A.dpad / MP_BK;
    const i64 per = (i64)MP_SB * MP_SB;
    const i64 total = (A.directed ? nS * nS : nS * (nS + 1) / 2) * per;
    const double inf = __builtin_huge_val();
    for (int q = tid; q < 512; q += 256) mask[q] = 0u;
    unsigned long long wsurv = 0;
    lds_sync();
    for (i64 t = blockIdx.x; t < total; t += gridDim.x) {
        i64 SI = 0, I, J;
        if (A.directed) {
            const i64 sb = t / per, loc = t - sb * per;
            I = (sb / nS) * MP_SB + loc / MP_SB;
            J = (sb % nS) * MP_SB + loc % MP_SB;
        } else {
            tile_from_linear(t, nS, SI, I, J);
        }
        if (I >= nT || J >= nT || (!A.directed && J < I)) continue; // uniform per workgroup
        const i64 i0 = I * MP_BM, j0 = J * MP_BN;
        d4 acc[4][4];
        gram_tile_128(A.Xc + (i64)wave * A.ldn + i0 + c2, A.Xc + (i64)wave * A.ldn + j0 + c2, A.ldn, A.ldn, nchunk, lds, acc, wave, c2,
                      wr, wc, lr, lk);
        // (gram_tile_128 ends behind a barrier, and every wave was done with the previous tile's rows before its first)
        if (tid < 128) {
            const i64 i = i0 + tid;
            const bool in = i < A.n;
            rqs[tid] = A.rn[i]; // rnorm is padded to ldn
            fos[tid] = in ? A.fo[i] : 0.0;
            lfs[tid] = in ? A.lfo[i] : -inf;
            rkey[tid] = link_row_key(A.h2, i);
        }
        lds_sync();
        // ---- the filter: acc[a][b][r] is row i0 + wr*64 + a*16 + lk + 4r, column j0 + wc*64 + b*16 + lr
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int jl = wc * 64 + b * 16 + lr;
            const i64 j = j0 + jl;
            const double rj = A.rn[j];
            if (j < A.n) {
                const double fij = A.fi[j], lfj = A.lfi[j];
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int il = wr * 64 + a * 16 + lk + 4 * r;
                        const i64 i = i0 + il;
                        if (!(A.directed ? (i != j && i < A.n) : i < j)) continue;
                        const double u = link_uniform<UMAT>(A, rkey[il], i, j);
                        if (!(u < (fos[il] * fij) * (1.0 + 1e-12))) continue; // stage 1
                        bool pass = true;
                        if (u >= 0x1p-100) { // stage 2
                            const double rs = rqs[il] + rj;
                            const double glo = fmax(gram_value(rqs[il], rj, acc[a][b][r]) - A.einfl * rs, 0.0);
                            const float xf = __builtin_amdgcn_sqrtf((float)(glo * A.inv_hi2)) * 0.99999904632568359375f; // 1 - 2^-20
                            const float B = fmaxf(1.0f - xf, 0.0f) + 0x1p-22f;
                            const double rhs = (lfs[il] + lfj) + A.alpha * (double)__builtin_amdgcn_logf(B) + A.slack;
                            pass = !((double)__builtin_amdgcn_logf((float)u) >= rhs);
                        }
                        if (pass) atomicOr(&mask[il * 4 + (jl >> 5)], 1u << (jl & 31));
                    }
            }
        }
        lds_sync();
        // ---- the survivors, row by row: wave w takes the rows w, w + 4, ...; lane l the candidates j0 + l and j0 + l + 64
        for (int rr = 0; rr < 32; rr++) {
            const int il = wave + 4 * rr;
            const uint4 mw = *reinterpret_cast<const uint4 *>(mask + il * 4);
            if ((mw.x | mw.y | mw.z | mw.w) == 0u) continue; // (wave-uniform)
            const i64 vi = i0 + il;
            const double fo = fos[il];
            const unsigned long long rk = rkey[il];
            if (lane < 4) mask[il * 4 + lane] = 0u;
            wsurv += (unsigned long long)(__popc(mw.x) + __popc(mw.y) + __popc(mw.z) + __popc(mw.w));
            const unsigned w0 = lane < 32 ? mw.x : mw.y, w1 = lane < 32 ? mw.z : mw.w;
            bool edge[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const i64 j = j0 + lane + 64 * h;
                edge[h] = false;
                if (((h ? w1 : w0) >> (lane & 31)) & 1u) {
                    const double p = link_p<EXP2>(A.Xr, A.d, vi, j, fo, A.fi[j], A.hi, A.alpha);
                    edge[h] = link_uniform<UMAT>(A, rk, vi, j) < p;
                }
            }
            const unsigned long long b0 = __ballot(edge[0]), b1 = __ballot(edge[1]);
            const int n0 = __popcll(b0), n1 = __popcll(b1);
            if (n0 + n1 == 0) continue;
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(A.cnt, (unsigned long long)(n0 + n1));
            at = __shfl(at, 0);
            const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const i64 pos = (i64)at + (h ? n0 + __popcll(b1 & below) : __popcll(b0 & below));
                if (edge[h] && pos < A.cap)
                    A.keys[pos] = ((unsigned long long)(unsigned)vi << 32) | (unsigned long long)(unsigned)(j0 + lane + 64 * h);
            }
        }
        // (the next tile's rows are written behind gram_tile_128's barriers: every wave has read its rows of the mask by then)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the cleared masks have landed before that barrier
    }
    if (lane == 0 && wsurv) atomicAdd(A.cnt + 1, wsurv);
}

// the sorted keys as 0-based int32 pairs (k_link_prob's operands) and 1-based int64 ids (the caller's)
__global__ void link_sample_unpack_kernel(const unsigned long long *__restrict__ keys, i64 ne, i32 *__restrict__ pi, i32 *__restrict__ pj,
                                          i64 *__restrict__ oi, i64 *__restrict__ oj) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += stride) {
        const unsigned long long key = keys[e];
        const i32 a = (i32)(key >> 32), b = (i32)(key & 0xffffffffull);
        pi[e] = a; pj[e] = b;
        oi[e] = (i64)a + 1; oj[e] = (i64)b + 1;
    }
}
__global__ void link_log2_kernel(const double *__restrict__ f, i64 cnt, double *__restrict__ lf) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < cnt) lf[v] = log2(f[v]);
}
void k_link_log_factors(cge_ctx *c) {
    LinkModel &m = c->link;
    if (m.lf_ready) return;
    m.lf.ensure((size_t)2 * m.n);
    hipLaunchKernelGGL(link_log2_kernel, dim3((unsigned)((2 * m.n + 255) / 256)), dim3(256), 0, c->stream, m.f.p, 2 * m.n, m.lf.p);
    m.lf_ready = true;
}

i64 k_link_sample(cge_ctx *c, i64 seed, i64 stream_id, unsigned long long *keys, i64 cap, unsigned long long *cnt, const double *U,
                  int ulay) {
    LinkModel &m = c->link;
    k_link_log_factors(c);
    const i64 nT = c->ldn / MP_BM;
    const i64 tiles = m.directed ? nT * nT : nT * (nT + 1) / 2;
    LinkSample A{};
    A.Xc = c->Xc.p; A.rn = c->rnorm.p; A.ldn = c->ldn; A.n = c->n; A.dpad = c->dpad;
    A.Xr = c->Xr.p; A.d = c->d;
    A.fo = m.f.p; A.fi = m.f.p + m.n; A.lfo = m.lf.p; A.lfi = m.lf.p + m.n;
    A.hi = m.hi; A.alpha = m.alpha;
    A.einfl = (double)(c->dpad + 16) * 2.220446049250313e-16; // (K + 16) 2^-52
    A.inv_hi2 = 1.0 / (m.hi * m.hi);
    A.slack = (1.0 + m.alpha) * 0x1p-14;
    A.directed = m.directed;
    A.h2 = cge_sm64(cge_sm64((uint64_t)seed ^ 0x6a09e667f3bcc909ULL) ^ ((uint64_t)stream_id * 0xd1342543de82ef95ULL + 1));
    A.U = U; A.ulay = ulay;
    A.keys = keys; A.cap = cap; A.cnt = cnt;
    const dim3 grid((unsigned)std::max<i64>(1, std::min<i64>(tiles, 2 * (i64)device_cus(c))));
    ScopedKernelTimer t(c, "link_sample");
#define LS_LAUNCH(E, UM)                                                                                                          \
    do {                                                                                                                           \
        cge_allow_lds((const void *)link_sample_kernel<E, UM>, LS_LDS_BYTES);                                                      \
        hipLaunchKernelGGL((link_sample_kernel<E, UM>), grid, dim3(256), LS_LDS_BYTES, c->stream, A);                              \
    } while (0)
    if (U) {
        if (m.pow_form) LS_LAUNCH(true, true);
        else LS_LAUNCH(false, true);
    } else {
        if (m.pow_form) LS_LAUNCH(true, false);
        else LS_LAUNCH(false, false);
    }
#undef LS_LAUNCH
    return tiles;
}
// the stored keys sorted and taken apart: pi / pj (0-based, for k_link_prob), oi / oj (1-based)
void k_link_sample_finish(cge_ctx *c, const unsigned long long *keys_in, unsigned long long *keys, i64 ne, i32 *pi, i32 *pj, i64 *oi,
                          i64 *oj) {
    if (ne <= 0) return;
    {
        ScopedKernelTimer t(c, "link_sample_sort");
        size_t bytes = 0;
        HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, keys_in, keys, (size_t)ne, 0u, 64u, c->stream));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::radix_sort_keys(c->sort_tmp.p, bytes, keys_in, keys, (size_t)ne, 0u, 64u, c->stream));
    }
    hipLaunchKernelGGL(link_sample_unpack_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c->stream, keys, ne, pi, pj, oi, oj);
}

// ---- cge_link_auc -----------------------------------------------------------------------------------------------------------------
// Every resident edge row e is a positive with the threshold p_e (k_link_prob's value), every non-edge a negative; per positive the
// negatives strictly below it and level with it.  The thresholds are sorted ascending once (t, with the permutation back to the
// edge list's order), and link_sample_kernel's walk of all pair tiles places every negative among them:
//   * the filter is link_rank_kernel's (link_filter_mask<true, true>: the candidate's own factor, both sides) with ONE pair of
//     thresholds for every row, t_min = t[0] and t_max = t[m - 1].  A pair it proves below t_min is below every positive, a pair
//     it proves above t_max is below none; neither can be a resident edge (an edge's own value is one of the thresholds, and the
//     filter never puts a value on the wrong side of one), so neither needs the edge keys.  Both are counted per lane and leave
//     the kernel in one atomic per wave;
//   * every other pair is evaluated with link_p.  Below t_min or above t_max it joins the two groups above.  Otherwise ub, the
//     first slot with t > p, takes one add of G (an inclusive prefix sum gives `less`), and when slots equal p exist -- lb < ub,
//     lb the first slot with t >= p -- the pair is a tie of that run (one add of E at the run's start) UNLESS it is a resident
//     edge: only here are the keys searched, since an edge's value always meets its own threshold.
// Integer atomics: the counts do not depend on the grid, the shares of the parts or the order.
struct LinkAuc : LinkTiles {
    const double *t; i64 m;            // the positives' values ascending
    unsigned long long *G, *E;         // per slot: negatives that are first below it / that equal its run (at the run's start)
    const double *fib;                 // f_in[c]^(-1 / alpha)
    int part, nparts;                  // this call walks the positions part, part + nparts, ... of the tile order
    unsigned long long *cnt;           // [0] pairs evaluated, [1] proven below t_min, [2] proven above t_max, [3] evaluated and
};                                     // below t_min, [4] tiles

template <bool EXP2>
__global__ __launch_bounds__(256, 2) void link_auc_kernel(LinkAuc A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *erow = lds + (size_t)2 * 2 * MP_BK * MP_LD, *arow = erow + 128, *asure = arow + 128, *rqs = asure + 128;
    unsigned *mask = reinterpret_cast<unsigned *>(rqs + 128);
    unsigned *mask2 = reinterpret_cast<unsigned *>(lds); // the pairs proven above t_max: in the Gram staging, free between two tiles
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4, c2 = lane * 2;
    const i64 nT = A.ldn / MP_BM, nS = (nT + MP_SB - 1) / MP_SB, nchunk = A.dpad / MP_BK;
    const i64 per = (i64)MP_SB * MP_SB;
    const i64 total = (A.directed ? nS * nS : nS * (nS + 1) / 2) * per;
    const double inf = __builtin_huge_val();
    const double tmin = A.t[0], tmax = A.t[A.m - 1];
    for (int q = tid; q < 512; q += 256) mask[q] = 0u;
    unsigned long long lsurv = 0, lbelow = 0, labove = 0, llow = 0, ntile = 0; // per lane; added up once, at the end
    lds_sync();
    for (i64 t = (i64)A.part + (i64)A.nparts * blockIdx.x; t < total; t += (i64)A.nparts * gridDim.x) {
        i64 SI = 0, I, J;
        if (A.directed) {
            const i64 sb = t / per, loc = t - sb * per;
            I = (sb / nS) * MP_SB + loc / MP_SB;
            J = (sb % nS) * MP_SB + loc % MP_SB;
        } else {
            tile_from_linear(t, nS, SI, I, J);
        }
        if (I >= nT || J >= nT || (!A.directed && J < I)) continue; // uniform per workgroup
        const i64 i0 = I * MP_BM, j0 = J * MP_BN;
        d4 acc[4][4];
        gram_tile_128(A.Xc + (i64)wave * A.ldn + i0 + c2, A.Xc + (i64)wave * A.ldn + j0 + c2, A.ldn, A.ldn, nchunk, lds, acc, wave, c2,
                      wr, wc, lr, lk);
        // (gram_tile_128 ends behind a barrier, and every wave was done with the previous tile's rows before its first)
        if (tid < 128) { // the rows' roots of t_min and t_max (link_root_row, link_root_row_sure); a row beyond n passes nothing
            const i64 i = i0 + tid;
            const double rq = A.rn[i]; // rnorm is padded to ldn
            double ar = inf, as = inf;
            if (i < A.n) {
                const double fo = A.fo[i];
                ar = link_root_row(tmin, fo, A.alpha);
                as = link_root_row_sure(tmax, fo, A.alpha);
            }
            rqs[tid] = rq;
            arow[tid] = ar;
            asure[tid] = as;
            erow[tid] = i < A.n ? A.einfl * rq : -inf;
        }
        for (int q = tid; q < 512; q += 256) mask2[q] = 0u;
        ntile++;
        lds_sync();
        link_filter_mask<true, true>(A, acc, j0, rqs, arow, erow, A.fib, mask, wr, wc, lr, lk, asure, mask2);
        lds_sync();
        // ---- row by row: wave w takes the rows w, w + 4, ...; lane l the candidates j0 + l and j0 + l + 64
        for (int rr = 0; rr < 32; rr++) {
            const int il = wave + 4 * rr;
            const i64 vi = i0 + il;
            const uint4 mw = *reinterpret_cast<const uint4 *>(mask + il * 4);
            const uint4 ms = *reinterpret_cast<const uint4 *>(mask2 + il * 4);
            if (lane < 4) mask[il * 4 + lane] = 0u;
            if (vi >= A.n) continue; // (wave-uniform)
            const unsigned w0 = lane < 32 ? mw.x : mw.y, w1 = lane < 32 ? mw.z : mw.w;
            const unsigned s0 = lane < 32 ? ms.x : ms.y, s1 = lane < 32 ? ms.z : ms.w;
            const double fo = A.fo[vi];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const i64 j = j0 + lane + 64 * h;
                if (!(j < A.n && (A.directed ? j != vi : vi < j))) continue; // not a pair of the model
                const bool on = (((h ? w1 : w0) >> (lane & 31)) & 1u) != 0u;
                const bool sure = (((h ? s1 : s0) >> (lane & 31)) & 1u) != 0u;
                if (!on) { lbelow++; continue; }
                if (sure) { labove++; continue; }
                lsurv++;
                const double p = link_p<EXP2>(A.Xr, A.d, vi, j, fo, A.fi[j], A.hi, A.alpha);
                if (!(p >= 0.0) || p > tmax) continue; // (a NaN: unspecified) above every positive
                if (p < tmin) { llow++; continue; }
                i64 lo = 0, hi = A.m; // lb: the first slot with t >= p
                while (lo < hi) {
                    const i64 mid = (lo + hi) >> 1;
                    if (A.t[mid] < p) lo = mid + 1;
                    else hi = mid;
                }
                const i64 lb = lo;
                hi = A.m; // ub: the first slot with t > p, from there on
                while (lo < hi) {
                    const i64 mid = (lo + hi) >> 1;
                    if (A.t[mid] <= p) lo = mid + 1;
                    else hi = mid;
                }
                if (lb < lo) { // level with a run of positives: one of them itself, if the pair is a resident edge
                    if (link_is_edge(A.keys, A.nkeys, link_key(vi, j, A.directed))) continue;
                    atomicAdd(A.E + lb, 1ull);
                }
                if (lo < A.m) atomicAdd(A.G + lo, 1ull);
            }
        }
        // (the next tile's staging is written behind gram_tile_128's first barrier: every wave has read its rows of mask2 by then)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the cleared masks have landed before that barrier
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lsurv += __shfl_xor(lsurv, s);
        lbelow += __shfl_xor(lbelow, s);
        labove += __shfl_xor(labove, s);
        llow += __shfl_xor(llow, s);
    }
    if (lane == 0) {
        if (lsurv) atomicAdd(A.cnt, lsurv);
        if (lbelow) atomicAdd(A.cnt + 1, lbelow);
        if (labove) atomicAdd(A.cnt + 2, labove);
        if (llow) atomicAdd(A.cnt + 3, llow);
        if (wave == 0 && ntile) atomicAdd(A.cnt + 4, ntile);
    }
}

// the distinct non-loop keys of the sorted edge keys: what the non-edges are counted from
__global__ void link_distinct_kernel(const unsigned long long *__restrict__ keys, i64 nkeys, unsigned long long *__restrict__ out) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    unsigned long long cnt = 0;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < nkeys; e += stride) {
        const unsigned long long key = keys[e];
        if (e > 0 && keys[e - 1] == key) continue;
        if ((key >> 32) != (key & 0xffffffffull)) cnt++;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out, cnt);
}
// G holds its inclusive prefix sum here: `less` of slot s is that plus the pairs below t_min, `ties` the E of the slot's run (equal
// thresholds -- repeated rows, symmetric configurations -- share both); written through the permutation to the edge list's order
__global__ void link_auc_final_kernel(const double *__restrict__ t, const i64 *__restrict__ perm, const unsigned long long *__restrict__ G,
                                      const unsigned long long *__restrict__ E, const unsigned long long *__restrict__ cnt, i64 m,
                                      i64 *__restrict__ out_less, i64 *__restrict__ out_ties) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const unsigned long long below = cnt[1] + cnt[3];
    for (i64 s = (i64)blockIdx.x * blockDim.x + threadIdx.x; s < m; s += stride) {
        const double ts = t[s];
        i64 lo = 0, hi = s; // the first slot of the run equal to ts
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (t[mid] < ts) lo = mid + 1;
            else hi = mid;
        }
        const i64 at = perm[s];
        out_less[at] = (i64)(G[s] + below);
        out_ties[at] = (i64)E[lo];
    }
}

// p: the positives' values in the edge list's order (k_link_prob's).  t / perm / G / E: m entries each; cnt: 6 counters (the
// kernel's five and the distinct non-loop keys); out_less / out_ties in the edge list's order.
void k_link_auc(cge_ctx *c, int part, int nparts, const double *p, double *t, i64 *perm, unsigned long long *G, unsigned long long *E,
                unsigned long long *cnt, i64 *out_less, i64 *out_ties) {
    LinkModel &m = c->link;
    const i64 ne = c->m;
    k_link_fib(c);
    HIP_CHECK(hipMemsetAsync(G, 0, sizeof(unsigned long long) * 2 * ne, c->stream)); // (G and E are one allocation)
    HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * 6, c->stream));
    {
        ScopedKernelTimer tm(c, "link_auc_sort"); // non-negative doubles: any order of the bits is the order of the values
        size_t bytes = 0;
        rocprim::counting_iterator<i64> iota(0);
        HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, p, t, iota, perm, (size_t)ne, 0u, 64u, c->stream));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::radix_sort_pairs(c->sort_tmp.p, bytes, p, t, iota, perm, (size_t)ne, 0u, 64u, c->stream));
    }
    hipLaunchKernelGGL(link_distinct_kernel, dim3(grid_for(m.nkeys, 256)), dim3(256), 0, c->stream, m.keys.p, m.nkeys, cnt + 5);
    const i64 nT = c->ldn / MP_BM, nS = (nT + MP_SB - 1) / MP_SB;
    const i64 total = (m.directed ? nS * nS : nS * (nS + 1) / 2) * MP_SB * MP_SB; // positions of the walk, padding included
    const i64 mine = total > part ? (total - part + nparts - 1) / nparts : 0;
    LinkAuc A{};
    A.Xc = c->Xc.p; A.rn = c->rnorm.p; A.ldn = c->ldn;
    A.n = c->n; A.dpad = c->dpad;
    A.Xr = c->Xr.p; A.d = c->d;
    A.fo = m.f.p; A.fi = m.f.p + m.n;
    A.hi = m.hi; A.alpha = m.alpha;
    A.einfl = (double)(c->dpad + 16) * 2.220446049250313e-16; // (K + 16) 2^-52
    A.dinfl = 1.0 + A.einfl;
    A.keys = m.keys.p; A.nkeys = m.nkeys; A.directed = m.directed;
    A.t = t; A.m = ne; A.G = G; A.E = E; A.fib = m.fib.p;
    A.part = part; A.nparts = nparts; A.cnt = cnt;
    const dim3 grid((unsigned)std::max<i64>(1, std::min<i64>(mine, 2 * (i64)device_cus(c))));
    {
        ScopedKernelTimer tm(c, "link_auc");
        if (m.pow_form) {
            cge_allow_lds((const void *)link_auc_kernel<true>, LR_LDS_BYTES);
            hipLaunchKernelGGL(link_auc_kernel<true>, grid, dim3(256), LR_LDS_BYTES, c->stream, A);
        } else {
            cge_allow_lds((const void *)link_auc_kernel<false>, LR_LDS_BYTES);
            hipLaunchKernelGGL(link_auc_kernel<false>, grid, dim3(256), LR_LDS_BYTES, c->stream, A);
        }
    }
    ScopedKernelTimer tm(c, "link_auc_final");
    size_t bytes = 0;
    HIP_CHECK(rocprim::inclusive_scan(nullptr, bytes, G, G, (size_t)ne, rocprim::plus<unsigned long long>(), c->stream));
    c->sort_tmp.ensure(bytes);
    HIP_CHECK(rocprim::inclusive_scan(c->sort_tmp.p, bytes, G, G, (size_t)ne, rocprim::plus<unsigned long long>(), c->stream));
    hipLaunchKernelGGL(link_auc_final_kernel, dim3(grid_for(ne, 256)), dim3(256), 0, c->stream, t, perm, G, E, cnt, ne, out_less,
                       out_ties);
}

// ---- cge_link_moments -------------------------------------------------------------------------------------------------------------
// The sums of the model over EVERY pair: per vertex the expected degrees, per community pair the expected edge mass B = sum p and
// the variance of a draw's edge count V = sum q (1 - q), q = min(p, 1).  The vertices are ordered by community first (host:
// stable, ids ascending inside a community) and the centred operand is gathered in that order (k_gather_centre_fm), so a
// 128 x 128 tile meets a handful of (row segment, column segment) rectangles, and in the undirected walk i < j by position has
// c_i <= c_j.
//
// Geometry, fixed by n alone.  The tiles are grouped in blocks of wb x wb (link_moments_wb(nT)); a WORK ITEM is one block (SI, SJ)
// -- undirected SJ >= SI and inside it only the tiles J >= I, in a diagonal tile only the pairs i < j.  Workgroups take items by
// stride; an item's partials are its own:
//   * rowp / colp: wb x 128 doubles each, the row sums and column sums of its tiles.  A row tile's sums are accumulated over the
//     item's column tiles in LDS by the thread of the row and stored once; a column's are added to the item's own global slot by
//     the thread of the column, tile after tile (one thread, one address: program order).
//   * Bp / Vp: one slot per (community of the row block, community of the column block) and WAVE; lane 0 of a wave adds its
//     rectangle sums to its own slot, tile after tile.
// Inside a tile every sum has a fixed shape: a lane adds its 16 x 4 values in index order, lanes are combined by xor butterflies,
// the two waves of a row (column) in wave order.  link_moments_deg_kernel / link_moments_bin_kernel add the items' partials per
// vertex and per bin in item order.  No floating-point atomic anywhere; device_cus() decides how many workgroups run, never which
// terms meet in which partial: the result is a function of the inputs alone.  The counters are integer atomics.
//
// Per pair: fast where safe, exact where not.  g is the Gram value, r_i, r_j the squared norms, e = (K + 16) 2^-52 the bound
// |g - d^2| <= e (r_i + r_j) derived at pcent_kernel (kernels_dist.hip).
//   (a) g - e (r_i + r_j) > hi^2 (1 + 1e-12): the distance is above hi by more than dist()'s own (K / 2 + 3) 2^-53, the base
//       is clamped, p = 0 exactly as link_p gives it (only under a supplied hi below the diameter);
//   (b) g >= theta (r_i + r_j) and b = 1 - sqrt(g) / hi >= beta, theta = beta = 2^-10: pw = pow(b, alpha).  g is within e / theta
//       of d^2 relatively, its root within e / (2 theta), x = d / hi <= 1 within the same absolutely, so the base is off by at most
//       e / (2 theta) (+ 3 ulp) and the power by  alpha e / (2 theta)  for alpha >= 1 (the derivative alpha b^(alpha - 1) <= alpha)
//       and  alpha (beta / 2)^(alpha - 1) e / (2 theta)  for alpha < 1 (both bases are above beta / 2).  At K = 512 that is
//       6e-11 alpha, resp. 6e-11 alpha (beta / 2)^(alpha - 1) = 4.6e-9 at alpha = 0.25.  (Against a reference that takes dist()
//       in fp64, that sum's own (d + 6) 2^-52 joins e: tests/link_moments_ref.py, 9.1e-9 at d = 512, alpha = 0.25);
//   (c) every other pair -- coincident and near points (g below theta (r_i + r_j): no relative bound), pairs at the diameter
//       (b below beta: the power's derivative is unbounded for alpha < 1) -- goes through link_p from the rows.
// The power is the library pow in every case.  The bound is ABSOLUTE per pair, c f_out[i] f_in[j]: a bin of far-apart
// communities has a tiny sum and the same tolerance per pair; that is what a Gram-based sum can promise.
//
// Registers: pow inlined 64 times over the accumulators is what spills link_topk_kernel's epilogue.  Here a wave parks a quarter
// of its accumulators (16 values a lane) in the Gram staging, free between two tiles, and a rolled loop of 16 evaluates them one
// at a time -- the only state across the loop is the three counters -- then takes the values back: four copies of pow in the
// code, not 64, and the 64 p live where the dot products lived.
struct LinkMoments {
    const double *Xp, *rp; i64 ldn, n, dpad; // the centred feature-major operand in community order, its squared norms
    const double *Xr; i64 d;                 // the rows as dist() reads them (original ids)
    const i32 *perm;                         // position -> vertex
    const double *fo, *fi;                   // the factors by position
    const i32 *rank;                         // by position: the community's rank among the communities present
    int wb; i64 nT, nB, items;               // tiles a block edge, tiles, blocks, work items
    const i32 *isi, *isj;                    // the items' blocks
    const i32 *bfr, *bnc;                    // per block: its first rank, its ranks
    const i64 *boff;                         // per item: its first bin slot
    double *rowp, *colp, *Bp, *Vp;
    unsigned long long *cnt;                 // [0] exact, [1] fast, [2] p > 1, [3] tiles
    double hi, hi2, alpha, einfl, theta, beta;
    int directed;
};
#define LM_LDS_BYTES ((size_t)2 * 2 * MP_BK * MP_LD * sizeof(double) + (size_t)(5 * 128 + 128) * sizeof(double))

__device__ __forceinline__ i64 link_moments_item(i64 SI, i64 SJ, i64 nB, int directed) {
    return directed ? SI * nB + SJ : SI * nB - SI * (SI - 1) / 2 + (SJ - SI);
}

__global__ __launch_bounds__(256, 2) void link_moments_kernel(LinkMoments A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *rqs = lds + (size_t)2 * 2 * MP_BK * MP_LD, *fos = rqs + 128, *rcs = fos + 128, *fis = rcs + 128, *racc = fis + 128;
    int *rkr = reinterpret_cast<int *>(racc + 128), *rkc = rkr + 128;
    double *rs = lds + 4096, *cs = rs + 256; // in the Gram staging, behind the waves' 4 x 1024 parked values
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4, c2 = lane * 2;
    const i64 nchunk = A.dpad / MP_BK;
    double *mybuf = lds + wave * 1024 + lane;
    unsigned long long nexact = 0, nfast = 0, nsat = 0, ntile = 0;
    for (i64 it = blockIdx.x; it < A.items; it += gridDim.x) {
        const i64 SI = A.isi[it], SJ = A.isj[it];
        const i64 I0 = SI * A.wb, I1 = I0 + A.wb < A.nT ? I0 + A.wb : A.nT;
        const i64 J0 = SJ * A.wb, J1 = J0 + A.wb < A.nT ? J0 + A.wb : A.nT;
        const int frI = A.bfr[SI], frJ = A.bfr[SJ], ncJ = A.bnc[SJ];
        const i64 slot0 = A.boff[it];
        for (i64 I = I0; I < I1; I++) {
            const i64 i0 = I * MP_BM;
            if (tid < 128) racc[tid] = 0.0; // (the thread's own: read and written by no other)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (i64 J = (!A.directed && I > J0) ? I : J0; J < J1; J++) {
                const i64 j0 = J * MP_BN;
                d4 acc[4][4];
                gram_tile_128(A.Xp + (i64)wave * A.ldn + i0 + c2, A.Xp + (i64)wave * A.ldn + j0 + c2, A.ldn, A.ldn, nchunk, lds, acc, wave,
                              c2, wr, wc, lr, lk);
                // (gram_tile_128 ends behind a barrier, and every wave was done with the previous tile's tables before its first)
                {
                    const int t = tid & 127;
                    const i64 v = (tid < 128 ? i0 : j0) + t;
                    const bool in = v < A.n;
                    const double r = A.rp[v]; // padded to ldn
                    if (tid < 128) {
                        rqs[t] = r;
                        fos[t] = in ? A.fo[v] : 0.0;
                        rkr[t] = in ? A.rank[v] : -1;
                    } else {
                        rcs[t] = r;
                        fis[t] = in ? A.fi[v] : 0.0;
                        rkc[t] = in ? A.rank[v] : -1;
                    }
                }
                if (tid == 0) ntile++;
                lds_sync();
                // ---- every pair's p: acc[a][b][r] is row i0 + wr*64 + a*16 + lk + 4r, column j0 + wc*64 + b*16 + lr
#pragma unroll
                for (int a = 0; a < 4; a++) {
#pragma unroll
                    for (int b = 0; b < 4; b++)
#pragma unroll
                        for (int r = 0; r < 4; r++) mybuf[(b * 4 + r) * 64] = acc[a][b][r];
#pragma unroll 1
                    for (int t = 0; t < 16; t++) {
                        const int il = wr * 64 + a * 16 + lk + 4 * (t & 3), jl = wc * 64 + (t >> 2) * 16 + lr;
                        const i64 i = i0 + il, j = j0 + jl;
                        double p = 0.0;
                        if (i < A.n && j < A.n && (A.directed ? i != j : i < j)) {
                            const double ri = rqs[il], rj = rcs[jl], rsum = ri + rj;
                            const double g = gram_value(ri, rj, mybuf[t * 64]);
                            const double fo = fos[il], fi = fis[jl];
                            double pw = 0.0;
                            bool fast = false;
                            if (g - A.einfl * rsum > A.hi2) {
                                fast = true; // (a)
                            } else if (g >= A.theta * rsum) {
                                const double bb = 1.0 - sqrt(g) / A.hi;
                                if (bb >= A.beta) { // (b)
                                    pw = pow(bb, A.alpha);
                                    fast = true;
                                }
                            }
                            if (fast) {
                                p = (fo * fi) * pw;
                                nfast++;
                            } else { // (c)
                                p = link_p<false>(A.Xr, A.d, A.perm[i], A.perm[j], fo, fi, A.hi, A.alpha);
                                nexact++;
                            }
                            if (p > 1.0) nsat++;
                        }
                        mybuf[t * 64] = p;
                    }
#pragma unroll
                    for (int b = 0; b < 4; b++)
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[a][b][r] = mybuf[(b * 4 + r) * 64];
                }
                // ---- row sums and column sums of the tile
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        double s = ((acc[a][0][r] + acc[a][1][r]) + acc[a][2][r]) + acc[a][3][r];
                        s += __shfl_xor(s, 1);
                        s += __shfl_xor(s, 2);
                        s += __shfl_xor(s, 4);
                        s += __shfl_xor(s, 8);
                        if (lr == 0) rs[wc * 128 + wr * 64 + a * 16 + lk + 4 * r] = s;
                    }
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    double s = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int r = 0; r < 4; r++) s += acc[a][b][r];
                    s += __shfl_xor(s, 16);
                    s += __shfl_xor(s, 32);
                    if (lk == 0) cs[wr * 128 + wc * 64 + b * 16 + lr] = s;
                }
                lds_sync();
                if (tid < 128) {
                    racc[tid] += rs[tid] + rs[128 + tid];
                } else {
                    const int t = tid - 128;
                    double *cp = A.colp + (it * A.wb + (J - J0)) * 128 + t;
                    *cp += cs[t] + cs[128 + t];
                }
                // ---- the rectangles of the tile: (rank of the rows) x (rank of the columns), each in the same fixed order
                {
                    const i64 nrow = A.n - i0 < 128 ? A.n - i0 : 128, ncol = A.n - j0 < 128 ? A.n - j0 : 128;
                    const int R0 = rkr[0], R1 = rkr[nrow - 1], C0 = rkc[0], C1 = rkc[ncol - 1];
                    int myr[4][4], myc[4];
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int r = 0; r < 4; r++) myr[a][r] = rkr[wr * 64 + a * 16 + lk + 4 * r];
#pragma unroll
                    for (int b = 0; b < 4; b++) myc[b] = rkc[wc * 64 + b * 16 + lr];
                    for (int R = R0; R <= R1; R++)
                        for (int Cc = (!A.directed && R > C0) ? R : C0; Cc <= C1; Cc++) {
                            double s = 0.0, v = 0.0;
#pragma unroll
                            for (int a = 0; a < 4; a++)
#pragma unroll
                                for (int b = 0; b < 4; b++)
#pragma unroll
                                    for (int r = 0; r < 4; r++) {
                                        const double pp = (myr[a][r] == R && myc[b] == Cc) ? acc[a][b][r] : 0.0;
                                        const double q = pp > 1.0 ? 1.0 : pp;
                                        s += pp;
                                        v += q * (1.0 - q);
                                    }
#pragma unroll
                            for (int w = 1; w < 64; w <<= 1) {
                                s += __shfl_xor(s, w);
                                v += __shfl_xor(v, w);
                            }
                            if (lane == 0) {
                                const i64 slot = (slot0 + (i64)(R - frI) * ncJ + (Cc - frJ)) * 4 + wave;
                                A.Bp[slot] += s;
                                A.Vp[slot] += v;
                            }
                        }
                }
                // (the next tile's staging is written behind gram_tile_128's first barrier: every wave has read rs / cs by then)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            if (tid < 128) A.rowp[(it * A.wb + (I - I0)) * 128 + tid] = racc[tid];
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        nexact += __shfl_xor(nexact, s);
        nfast += __shfl_xor(nfast, s);
        nsat += __shfl_xor(nsat, s);
    }
    if (lane == 0) {
        if (nexact) atomicAdd(A.cnt, nexact);
        if (nfast) atomicAdd(A.cnt + 1, nfast);
        if (nsat) atomicAdd(A.cnt + 2, nsat);
        if (wave == 0 && ntile) atomicAdd(A.cnt + 3, ntile);
    }
}

// the degrees: per position the items' row partials in item order, then their column partials; written to the vertex's own id
__global__ void link_moments_deg_kernel(LinkMoments A, double *__restrict__ deg_out, double *__restrict__ deg_in) {
    const i64 pos = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= A.n) return;
    const i64 stride = (i64)A.wb * 128, S = pos / stride, off = pos - S * stride;
    double ro = 0.0, co = 0.0;
    for (i64 SJ = A.directed ? 0 : S; SJ < A.nB; SJ++) ro += A.rowp[link_moments_item(S, SJ, A.nB, A.directed) * stride + off];
    for (i64 SI = 0; SI < (A.directed ? A.nB : S + 1); SI++) co += A.colp[link_moments_item(SI, S, A.nB, A.directed) * stride + off];
    const i64 v = A.perm[pos];
    if (A.directed) {
        deg_out[v] = ro;
        deg_in[v] = co;
    } else {
        deg_out[v] = ro + co;
    }
}
// the bins: one thread per pair of present communities (ranks ra, rb; undirected ra <= rb) adds the slots of the items that hold
// it, in item order and wave order, and writes the sweep's layout (cge_idx undirected, (c_i - 1) C + c_j directed)
__global__ void link_moments_bin_kernel(LinkMoments A, i64 Cp, i64 C, const i32 *__restrict__ cid, const i32 *__restrict__ rb0,
                                        const i32 *__restrict__ rb1, double *__restrict__ B, double *__restrict__ V) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Cp * Cp) return;
    const i64 ra = t / Cp, rb = t - ra * Cp;
    if (!A.directed && ra > rb) return;
    double b = 0.0, v = 0.0;
    for (i64 SI = rb0[ra]; SI <= rb1[ra]; SI++)
        for (i64 SJ = rb0[rb]; SJ <= rb1[rb]; SJ++) {
            if (!A.directed && SJ < SI) continue;
            const i64 it = link_moments_item(SI, SJ, A.nB, A.directed);
            const i64 slot = (A.boff[it] + (ra - A.bfr[SI]) * (i64)A.bnc[SJ] + (rb - A.bfr[SJ])) * 4;
            for (int w = 0; w < 4; w++) {
                b += A.Bp[slot + w];
                v += A.Vp[slot + w];
            }
        }
    const i64 ca = cid[ra], cb = cid[rb];
    const i64 at = A.directed ? ca * C + cb : C * ca - ca * (ca - 1) / 2 + (cb - ca);
    B[at] = b;
    V[at] = v;
}
__global__ void link_moments_permute_kernel(const double *__restrict__ f, const i32 *__restrict__ perm, i64 n, double *__restrict__ fs) {
    const i64 pos = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    fs[pos] = f[perm[pos]];
    fs[n + pos] = f[n + perm[pos]];
}

// tiles a block edge: 2 while that keeps the blocks under 512 a side, else the power of two that does (16 at n = 10^6)
i64 k_link_moments_wb(i64 nT) {
    i64 wb = 2;
    while ((nT + wb - 1) / wb > 512) wb *= 2;
    return wb;
}
// T (link_host.cpp) holds the tables of the call, already on the device; the partials are zeroed here.  deg / B / V: device outputs
// (deg: n, or 2 n directed; B, V: L each, zeroed here: a bin no pair falls in stays 0)
void k_link_moments(cge_ctx *c, const LinkMomentsTables &T, double *deg, double *B, double *V, i64 L, unsigned long long *cnt) {
    LinkModel &m = c->link;
    const i64 n = m.n;
    hipStream_t st = c->stream;
    k_gather_centre_fm(c, c->Xr.p, T.perm, c->gmean.p, m.mXp.p, m.mrp.p, n, c->d, c->ldn, c->dpad);
    hipLaunchKernelGGL(link_moments_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m.f.p, T.perm, n, m.mf.p);
    HIP_CHECK(hipMemsetAsync(m.mrow.p, 0, sizeof(double) * 2 * T.items * T.wb * 128, st));
    HIP_CHECK(hipMemsetAsync(m.mbin.p, 0, sizeof(double) * 8 * T.slots, st));
    HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * 4, st));
    HIP_CHECK(hipMemsetAsync(B, 0, sizeof(double) * L, st));
    HIP_CHECK(hipMemsetAsync(V, 0, sizeof(double) * L, st));
    LinkMoments A{};
    A.Xp = m.mXp.p; A.rp = m.mrp.p; A.ldn = c->ldn; A.n = n; A.dpad = c->dpad;
    A.Xr = c->Xr.p; A.d = c->d;
    A.perm = T.perm; A.fo = m.mf.p; A.fi = m.mf.p + n; A.rank = T.rank;
    A.wb = (int)T.wb; A.nT = T.nT; A.nB = T.nB; A.items = T.items;
    A.isi = T.isi; A.isj = T.isj; A.bfr = T.bfr; A.bnc = T.bnc; A.boff = T.boff;
    A.rowp = m.mrow.p; A.colp = m.mrow.p + T.items * T.wb * 128;
    A.Bp = m.mbin.p; A.Vp = m.mbin.p + 4 * T.slots;
    A.cnt = cnt;
    A.hi = m.hi; A.hi2 = m.hi * m.hi * (1.0 + 1e-12); A.alpha = m.alpha;
    A.einfl = (double)(c->dpad + 16) * 2.220446049250313e-16; // (K + 16) 2^-52
    A.theta = 0x1p-10; A.beta = 0x1p-10;
    A.directed = m.directed;
    const dim3 grid((unsigned)std::max<i64>(1, std::min<i64>(T.items, 2 * (i64)device_cus(c))));
    {
        ScopedKernelTimer t(c, "link_moments");
        cge_allow_lds((const void *)link_moments_kernel, LM_LDS_BYTES);
        hipLaunchKernelGGL(link_moments_kernel, grid, dim3(256), LM_LDS_BYTES, st, A);
    }
    ScopedKernelTimer t(c, "link_moments_final");
    hipLaunchKernelGGL(link_moments_deg_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, deg, deg + n);
    const i64 cc = T.Cp * T.Cp;
    hipLaunchKernelGGL(link_moments_bin_kernel, dim3((unsigned)((cc + 255) / 256)), dim3(256), 0, st, A, T.Cp, T.C, T.cid, T.rb0, T.rb1,
                       B, V);
}
