// kernels_link.hip -- the link model's kernels (cge_link_*, link_host.cpp): the per-vertex factors of a fitted model, the model's
// probability of given pairs, and per query the k most probable candidates.  gfx950 only.
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
#include "pow_parts.hpp"

#include <rocprim/rocprim.hpp>

#define LK_KMAX 64
#define LK_MAX_SLICES 512 // the merge kernel keeps nsl / 64 <= 8 list heads per lane
#define LK_EXTRA_DOUBLES (128 /* tau */ + 128 /* thr */ + 256 /* mask: 128 x 4 words */ + 64 /* counts: 128 ints */ + 128 /* rq */)
#define LK_LDS_BYTES ((size_t)2 * 2 * MP_BK * MP_LD * sizeof(double) + (size_t)LK_EXTRA_DOUBLES * sizeof(double))

// dist(i, j) of the resident rows in pair_dist_kernel's arithmetic: ascending k, unfused; 0 for equal indices
__device__ __forceinline__ double link_dist(const double *__restrict__ Xr, i64 d, i64 i, i64 j) {
    if (i == j) return 0.0;
    const double *a = Xr + i * d, *b = Xr + j * d;
    double s = 0.0;
    for (i64 q = 0; q < d; q++) {
        const double df = __dsub_rn(a[q], b[q]);
        s = __dadd_rn(s, __dmul_rn(df, df));
    }
    return sqrt(s);
}
// the power of the model: EXP2 = the per-element chain of the power matrix (log_parts + exp2_parts), else the library pow as
// auc_landmark_kernel takes it; the base clamped at 0 (x > 1: only under a supplied hi below the diameter)
template <bool EXP2>
__device__ __forceinline__ double link_power(double x, double alpha) {
    if (EXP2) {
        double Lh;
        float Ll;
        log_parts(x > 1.0 ? 1.0 : x, Lh, Ll);
        return exp2_parts(alpha, Lh, Ll);
    }
    const double b = 1.0 - x;
    return pow(b < 0.0 ? 0.0 : b, alpha);
}
template <bool EXP2>
__device__ __forceinline__ double link_p(const double *__restrict__ Xr, i64 d, i64 i, i64 j, double fo, double fi, double hi,
                                         double alpha) {
    const double x = link_dist(Xr, d, i, j) / hi;
    return (fo * fi) * link_power<EXP2>(x, alpha);
}

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
struct LinkTopk {
    const double *Xq, *rq; i64 ldq;   // the queries, centred feature-major (dpad x ldq) and their squared norms
    const double *Xc, *rn; i64 ldn;   // the candidates: every vertex, the same form
    i64 n, Q, dpad;
    int k, nsl;
    const i32 *qid;                    // the queries' vertex ids (Q)
    const double *Xr; i64 d;           // the rows as dist() reads them
    const double *fo, *fi, *ftile;
    double hi, alpha, einfl, dinfl;
    const unsigned long long *keys; i64 nkeys; int directed; // keys == nullptr: nothing is excluded
    double *lp; i32 *lj, *lcnt;        // the lists: [(row tile * nsl + slice) * 128 + row][k], and their lengths
    unsigned long long *surv;          // pairs evaluated exactly (a stat)
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

__device__ __forceinline__ void lds_sync() { // (the LDS stores of this wave have landed before the barrier: tests/test_device_asm.py)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
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
        // this tile's thresholds from the rows' tau and the tile's largest f_in, the rows' share of the rounding bound added
        if (tid < 128) {
            const i64 qi = i0 + tid;
            double t = -__builtin_huge_val();
            if (qi < A.Q) t = link_radius2(tau[tid], A.fo[A.qid[qi]] * A.ftile[J], A.hi, A.alpha, A.dinfl) + A.einfl * rqs[tid];
            thr[tid] = t;
        }
        lds_sync();
        // ---- the filter: acc[a][b][r] is row i0 + wr*64 + a*16 + lk + 4r, column j0 + wc*64 + b*16 + lr
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int jl = wc * 64 + b * 16 + lr;
            const i64 j = j0 + jl;
            const double rj = A.rn[j]; // rnorm is padded to ldn
            const double ej = A.einfl * rj;
            if (j < A.n) {
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int il = wr * 64 + a * 16 + lk + 4 * r;
                        const double g = gram_value(rqs[il], rj, acc[a][b][r]);
                        if (g <= thr[il] + ej) atomicOr(&mask[il * 4 + (jl >> 5)], 1u << (jl & 31));
                    }
            }
        }
        lds_sync();
        // ---- the survivors, row by row: wave w takes the rows w, w + 4, ...
        for (int rr = 0; rr < 32; rr++) {
            const int il = wave + 4 * rr;
            const uint4 mw = *reinterpret_cast<const uint4 *>(mask + il * 4);
            if ((mw.x | mw.y | mw.z | mw.w) == 0u) continue; // (wave-uniform)
            const i64 vi = A.qid[i0 + il]; // (a row beyond Q has an empty mask: its threshold is -inf)
            const double fo = A.fo[vi];
            const unsigned w0 = lane < 32 ? mw.x : mw.y, w1 = lane < 32 ? mw.z : mw.w;
            double pc[2];
            i32 jc[2];
            int nsurv = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const i64 j = j0 + lane + 64 * h;
                bool on = (((h ? w1 : w0) >> (lane & 31)) & 1u) != 0u;
                nsurv += on ? 1 : 0;
                on = on && j != vi;
                if (on && A.keys) on = !link_is_edge(A.keys, A.nkeys, link_key(vi, j, A.directed));
                pc[h] = on ? link_p<EXP2>(A.Xr, A.d, vi, j, fo, A.fi[j], A.hi, A.alpha) : -1.0;
                jc[h] = (i32)j;
            }
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
    i64 nsl = (2 * (i64)device_cus() + nQt - 1) / nQt;
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
