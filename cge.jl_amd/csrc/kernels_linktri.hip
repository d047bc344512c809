// kernels_linktri.hip -- expected and observed triangles of the link model (cge_link_triangles, link_host.cpp).  gfx950 only.
//
// Model side.  q(i, j) = min(p(i, j), 1) is what cge_link_sample draws with; Q is the symmetric n x n matrix of the q, zero on the
// diagonal, stored row-major with leading dimension ld = an ODD number of 128-tiles (k_link_tri_ld: a k-row step of a large power
// of two would put every k-row of a tile on the same channels), zero beyond n.
//   link_q_kernel     Q tile by tile: tile_dist2 (dist_tile.hpp) sums a pair's squared distance in link_dist's order, link_p_dist
//                     (link_p.hpp) is link_p's own tail, so an entry has cge_link_prob's bits; upper 64 x 64 tiles, mirrored.
//   link_tri_kernel   T = rowsum(Q o (Q Q)) without storing Q Q: max_pair_kernel's walk of the upper 128 x 128 tiles, each one
//                     gram_tile_128 (mfma_tile.hpp) with BOTH operands taken from Q (k-rows of Q, column blocks I and J: Q is
//                     symmetric, so sum_k Q[k][i] Q[k][j] = (Q Q)_ij) over ld-free nT * 8 chunks.  The epilogue multiplies the
//                     accumulators by the Q_IJ tile and reduces rows (block I's partial of "other block" J) and, off the diagonal,
//                     columns (block J's partial of "other block" I).  Every slot part[B][other][128] is written by exactly one tile.
//   link_tri_final_kernel  t[v] = (sum over `other` ascending of part[B(v)][other][v % 128]) / 2.
//   link_wedge_kernel w[i] = sum_k q_ik (sum_{j<k} q_ij): the pairs j < k of row i one by one, NO cancellation (the form
//                     (s1^2 - s2) / 2 has relative error s1^2 / (s1^2 - s2), unbounded for a row with one entry).
// All sums run in an order fixed by n alone (in-thread, butterfly, LDS pair, partial chain): no floating-point atomics, identical
// arrays at any grid.  Error: DESIGN.md section 4.17.
//
// Graph side.  The model's sorted undirected keys (k_link_keys: min << 32 | max) lose loops and repeats, every kept edge is oriented
// from its endpoint lower in (distinct degree, id) to the higher one, the oriented keys are sorted (per source: targets ascending)
// and every oriented edge u -> v intersects the lists of u and v: a common w closes the triangle {u, v, w}, found ONCE (at its
// lowest edge).  One lane per edge merges two short lists; when either list is longer than TRI_WAVE_THR the edge goes to a list
// that a second kernel serves one wave per edge (lanes stride the shorter list, binary search in the longer).  Integer atomics
// credit the three vertices: integer sums do not depend on the order.
#include "mfma_tile.hpp"
#include "dist_tile.hpp"
#include "link_p.hpp"

#include <rocprim/rocprim.hpp>

#define TRI_WAVE_THR 64 // oriented lists longer than this are intersected by a whole wave
#define LT_LDS_BYTES ((size_t)2 * 2 * MP_BK * MP_LD * sizeof(double) + (size_t)(4 * 128) * sizeof(double))

i64 k_link_tri_ld(i64 n) { return (((n + 127) / 128) | 1) * 128; }

// ---- Q -----------------------------------------------------------------------------------------------------------------------------
template <bool EXP2>
__global__ __launch_bounds__(256) void link_q_kernel(const double *__restrict__ Xr, i64 n, i64 d, const double *__restrict__ f,
                                                     double hi, double alpha, double *__restrict__ Q, i64 ld,
                                                     unsigned long long *__restrict__ sat) {
    __shared__ double As[DT][DK + 1], Bs[DT][DK + 1];
    __shared__ int scnt;
    const i64 bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return; // upper triangle of tiles; the mirror is written by the same block
    if (threadIdx.x == 0) scnt = 0;
    const i64 i0 = bi * DT, j0 = bj * DT;
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    double acc[4][4];
    tile_dist2(Xr, n, d, i0, j0, ty, tx, As, Bs, acc); // (its barriers also publish scnt = 0; d >= 1)
    int cnt = 0;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const i64 i = i0 + ty * 4 + a, j = j0 + tx * 4 + b; // (both below ld: the grid is ld / 64 square)
            double v = 0.0;
            if (i < n && j < n && i != j) {
                const double p = link_p_dist<EXP2>(sqrt(acc[a][b]), f[i], f[j], hi, alpha);
                v = p > 1.0 ? 1.0 : p;
                cnt += (p > 1.0 && i < j);
            }
            Q[i * ld + j] = v;
            if (bi != bj) Q[j * ld + i] = v;
        }
    if (cnt) atomicAdd(&scnt, cnt);
    lds_sync();
    if (threadIdx.x == 0 && scnt) atomicAdd(sat, (unsigned long long)scnt);
}

void k_link_tri_q(cge_ctx *c, double *Q, i64 ld, unsigned long long *sat) {
    const LinkModel &m = c->link;
    ScopedKernelTimer t(c, "link_tri_q");
    HIP_CHECK(hipMemsetAsync(sat, 0, sizeof(unsigned long long), c->stream));
    const unsigned nb = (unsigned)(ld / DT);
    if (m.pow_form)
        hipLaunchKernelGGL(link_q_kernel<true>, dim3(nb, nb), dim3(256), 0, c->stream, c->Xr.p, m.n, c->d, m.f.p, m.hi, m.alpha, Q, ld,
                           sat);
    else
        hipLaunchKernelGGL(link_q_kernel<false>, dim3(nb, nb), dim3(256), 0, c->stream, c->Xr.p, m.n, c->d, m.f.p, m.hi, m.alpha, Q, ld,
                           sat);
}

// ---- T = rowsum(Q o (Q Q)) -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void link_tri_kernel(const double *__restrict__ Q, i64 ld, i64 nT, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *rowb = lds + (size_t)2 * 2 * MP_BK * MP_LD, *colb = rowb + 256; // [2][128] each: the two waves that share a row / column
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4, c2 = lane * 2;
    const i64 nS = (nT + MP_SB - 1) / MP_SB;
    const i64 total = nS * (nS + 1) / 2 * MP_SB * MP_SB;
    const i64 nchunk = nT * (MP_BM / MP_BK); // the k-rows below nT * 128 (the rows beyond are zero)
    for (i64 t = blockIdx.x; t < total; t += gridDim.x) {
        i64 SI, I, J;
        tile_from_linear(t, nS, SI, I, J);
        if (I >= nT || J >= nT || J < I) continue; // uniform per workgroup
        const i64 i0 = I * MP_BM, j0 = J * MP_BN;
        d4 acc[4][4];
        gram_tile_128(Q + (i64)wave * ld + i0 + c2, Q + (i64)wave * ld + j0 + c2, ld, ld, nchunk, lds, acc, wave, c2, wr, wc, lr, lk);
        // acc[a][b][r]: row = i0 + wr*64 + a*16 + lk + 4r, col = j0 + wc*64 + b*16 + lr
        // the Hadamard product in place (the accumulators fill the register file: no second set of sums beside them)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const double *qc = Q + (i0 + wr * 64 + lk) * ld + j0 + wc * 64 + b * 16 + lr;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[a][b][r] *= qc[(i64)(a * 16 + 4 * r) * ld];        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                double v = ((acc[a][0][r] + acc[a][1][r]) + acc[a][2][r]) + acc[a][3][r]; // this lane's 4 columns, then the 16 lanes that share lk
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                v += __shfl_xor(v, 8);
                if (lr == 0) rowb[wc * 128 + wr * 64 + a * 16 + lk + 4 * r] = v;
            }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double v = 0.0; // this lane's 16 rows in (a, r) order, then the 4 row groups of the lanes that share lr
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int r = 0; r < 4; r++) v += acc[a][b][r];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lk == 0) colb[wr * 128 + wc * 64 + b * 16 + lr] = v;
        }
        lds_sync();
        if (tid < 128) part[((I * nT + J) * 128) + tid] = rowb[tid] + rowb[128 + tid];
        else if (J > I) part[((J * nT + I) * 128) + (tid - 128)] = colb[tid - 128] + colb[tid];
        // (rowb / colb are rewritten behind the barriers of the next tile's gram_tile_128)
    }
}
__global__ void link_tri_final_kernel(const double *__restrict__ part, i64 n, i64 nT, double *__restrict__ tri) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const double *p = part + (v / 128) * nT * 128 + (v % 128);
    double s = 0.0;
    for (i64 o = 0; o < nT; o++) s += p[o * 128];
    tri[v] = 0.5 * s;
}
// thread i walks column i of Q (= row i: symmetric), coalesced over the threads
__global__ __launch_bounds__(64) void link_wedge_kernel(const double *__restrict__ Q, i64 ld, i64 n, double *__restrict__ wed) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double w = 0.0, s = 0.0;
#pragma unroll 8 // (eight loads in flight; the additions keep their order)
    for (i64 k = 0; k < n; k++) {
        const double q = Q[k * ld + i];
        w += q * s;
        s += q;
    }
    wed[i] = w;
}

i64 k_link_tri_expected(cge_ctx *c, const double *Q, i64 ld, double *part, double *tri, double *wed) {
    const i64 n = c->link.n, nT = (n + 127) / 128;
    const i64 nS = (nT + MP_SB - 1) / MP_SB, total = nS * (nS + 1) / 2 * MP_SB * MP_SB;
    hipStream_t st = c->stream;
    if (tri) {
        const dim3 grid((unsigned)std::max<i64>(1, std::min<i64>(total, 2 * (i64)device_cus(c))));
        {
            ScopedKernelTimer t(c, "link_tri");
            cge_allow_lds((const void *)link_tri_kernel, LT_LDS_BYTES);
            hipLaunchKernelGGL(link_tri_kernel, grid, dim3(256), LT_LDS_BYTES, st, Q, ld, nT, part);
        }
        ScopedKernelTimer t(c, "link_tri_final");
        hipLaunchKernelGGL(link_tri_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, n, nT, tri);
    }
    if (wed) {
        ScopedKernelTimer t(c, "link_wedge");
        hipLaunchKernelGGL(link_wedge_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, Q, ld, n, wed);
    }
    return tri ? nT * (nT + 1) / 2 : 0;
}

// ---- observed triangles ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tri_kept(const unsigned long long *__restrict__ keys, i64 e) { // no loop, the first of its repeats
    const unsigned long long k = keys[e];
    return (unsigned)(k >> 32) != (unsigned)k && (e == 0 || keys[e - 1] != k);
}
__global__ void tri_degree_kernel(const unsigned long long *__restrict__ keys, i64 nk, i32 *__restrict__ deg) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < nk; e += stride) {
        if (!tri_kept(keys, e)) continue;
        atomicAdd(&deg[(unsigned)(keys[e] >> 32)], 1);
        atomicAdd(&deg[(unsigned)keys[e]], 1);
    }
}
__global__ void tri_orient_kernel(const unsigned long long *__restrict__ keys, i64 nk, const i32 *__restrict__ deg,
                                  unsigned long long *__restrict__ okeys) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < nk; e += stride) {
        unsigned long long o = ~0ull; // a dropped row sorts behind every edge
        if (tri_kept(keys, e)) {
            const unsigned a = (unsigned)(keys[e] >> 32), b = (unsigned)keys[e]; // a < b
            const i32 da = deg[a], db = deg[b];
            o = da <= db ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
        }
        okeys[e] = o;
    }
}
// off[u] = the first oriented edge whose source is >= u, u = 0 .. n (off[n] = the oriented edges: the dropped rows are behind)
__global__ void tri_offsets_kernel(const unsigned long long *__restrict__ okeys, i64 nk, i64 n, i64 *__restrict__ off) {
    const i64 u = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u > n) return;
    const unsigned long long key = (unsigned long long)u << 32;
    i64 lo = 0, hi = nk;
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (okeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    off[u] = lo;
}
// one lane per oriented edge: short lists are merged here, an edge with a long list is appended to `lng`
__global__ void tri_lane_kernel(const unsigned long long *__restrict__ okeys, const i64 *__restrict__ off, i64 n,
                                unsigned long long *__restrict__ tri, i64 *__restrict__ lng, unsigned long long *__restrict__ nlng) {
    const i64 ne = off[n], stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += stride) {
        const i64 u = (i64)(okeys[e] >> 32), v = (i64)(unsigned)okeys[e];
        i64 pu = off[u], pv = off[v];
        const i64 eu = off[u + 1], ev = off[v + 1];
        if (eu - pu > TRI_WAVE_THR || ev - pv > TRI_WAVE_THR) {
            lng[atomicAdd(nlng, 1ull)] = e;
            continue;
        }
        unsigned long long cnt = 0;
        while (pu < eu && pv < ev) {
            const unsigned x = (unsigned)okeys[pu], y = (unsigned)okeys[pv];
            if (x == y) {
                atomicAdd(&tri[x], 1ull);
                cnt++;
            }
            pu += x <= y;
            pv += y <= x;
        }
        if (cnt) {
            atomicAdd(&tri[u], cnt);
            atomicAdd(&tri[v], cnt);
        }
    }
}
// one wave per listed edge: the lanes stride the shorter list and look each target up in the longer
__global__ __launch_bounds__(256) void tri_wave_kernel(const unsigned long long *__restrict__ okeys, const i64 *__restrict__ off,
                                                       unsigned long long *__restrict__ tri, const i64 *__restrict__ lng,
                                                       const unsigned long long *__restrict__ nlng) {
    const i64 nl = (i64)*nlng, waves = (i64)gridDim.x * (blockDim.x >> 6);
    const int lane = threadIdx.x & 63;
    for (i64 q = (i64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < nl; q += waves) {
        const i64 e = lng[q];
        const i64 u = (i64)(okeys[e] >> 32), v = (i64)(unsigned)okeys[e];
        i64 s0 = off[u], s1 = off[u + 1], l0 = off[v], l1 = off[v + 1];
        if (s1 - s0 > l1 - l0) {
            i64 t0 = s0, t1 = s1;
            s0 = l0; s1 = l1; l0 = t0; l1 = t1;
        }
        unsigned long long cnt = 0;
        for (i64 p = s0 + lane; p < s1; p += 64) {
            const unsigned x = (unsigned)okeys[p];
            const unsigned long long key = (okeys[l0] & 0xFFFFFFFF00000000ull) | x;
            i64 lo = l0, hi = l1;
            while (lo < hi) {
                const i64 mid = (lo + hi) >> 1;
                if (okeys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            if (lo < l1 && okeys[lo] == key) {
                atomicAdd(&tri[x], 1ull);
                cnt++;
            }
        }
        if (cnt) {
            atomicAdd(&tri[u], cnt);
            atomicAdd(&tri[v], cnt);
        }
    }
}

// deg (n), tri (n): device outputs, zeroed here; okeys_in / okeys / lng: c->m entries each; off: n + 1; nlng: one counter
void k_link_tri_observed(cge_ctx *c, i32 *deg, unsigned long long *tri, unsigned long long *okeys_in, unsigned long long *okeys,
                         i64 *off, i64 *lng, unsigned long long *nlng) {
    LinkModel &m = c->link;
    k_link_keys(c);
    const i64 n = m.n, nk = m.nkeys;
    hipStream_t st = c->stream;
    ScopedKernelTimer t(c, "link_tri_observed");
    HIP_CHECK(hipMemsetAsync(deg, 0, sizeof(i32) * n, st));
    HIP_CHECK(hipMemsetAsync(tri, 0, sizeof(unsigned long long) * n, st));
    HIP_CHECK(hipMemsetAsync(nlng, 0, sizeof(unsigned long long), st));
    const dim3 ge(grid_for(nk, 256));
    hipLaunchKernelGGL(tri_degree_kernel, ge, dim3(256), 0, st, m.keys.p, nk, deg);
    hipLaunchKernelGGL(tri_orient_kernel, ge, dim3(256), 0, st, m.keys.p, nk, deg, okeys_in);
    size_t bytes = 0;
    HIP_CHECK(rocprim::radix_sort_keys(nullptr, bytes, okeys_in, okeys, (size_t)nk, 0u, 64u, st));
    c->sort_tmp.ensure(bytes);
    HIP_CHECK(rocprim::radix_sort_keys(c->sort_tmp.p, bytes, okeys_in, okeys, (size_t)nk, 0u, 64u, st));
    hipLaunchKernelGGL(tri_offsets_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, okeys, nk, n, off);
    hipLaunchKernelGGL(tri_lane_kernel, ge, dim3(256), 0, st, okeys, off, n, tri, lng, nlng);
    hipLaunchKernelGGL(tri_wave_kernel, dim3((unsigned)(4 * device_cus(c))), dim3(256), 0, st, okeys, off, tri, lng, nlng);
}
