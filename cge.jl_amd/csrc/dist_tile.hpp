// dist_tile.hpp -- the sequential-sum distance tile shared by the landmark-level D, the packed form of an exact sweep
// (kernels_dist.hip) and the link model's matrix Q (kernels_linktri.hip).  gfx950 only.
#pragma once
#include "common.hpp"

// 64x64 output tile per workgroup of 256, each thread a 4x4 sub-tile; operands staged through LDS in k-chunks; the k-sum runs in
// ascending k with unfused sub/mul/add, i.e. the arithmetic of dist() (src/auxilary.jl:14-20) term for term.
#define DT 64
#define DK 16
// The squared distances of the 64 x 64 tile at (i0, j0), thread (ty, tx) its 4 x 4 sub-tile: shared by every kernel that stores
// distances, so that all of them add the same terms in the same order.
__device__ __forceinline__ void tile_dist2(const double *__restrict__ emb, i64 N, i64 d, i64 i0, i64 j0, int ty, int tx,
                                           double (*As)[DK + 1], double (*Bs)[DK + 1], double acc[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
    for (i64 k0 = 0; k0 < d; k0 += DK) {
        __syncthreads();
        for (int e = threadIdx.x; e < DT * DK; e += 256) {
            const int r = e / DK, kk = e % DK;
            const i64 k = k0 + kk;
            As[r][kk] = (i0 + r < N && k < d) ? emb[(i0 + r) * d + k] : 0.0;
            Bs[r][kk] = (j0 + r < N && k < d) ? emb[(j0 + r) * d + k] : 0.0;
        }
        __syncthreads();
        const int kmax = (int)min((i64)DK, d - k0);
        for (int kk = 0; kk < kmax; kk++) {
            double a4[4], b4[4];
#pragma unroll
            for (int a = 0; a < 4; a++) a4[a] = As[ty * 4 + a][kk];
#pragma unroll
            for (int b = 0; b < 4; b++) b4[b] = Bs[tx * 4 + b][kk];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const double df = __dsub_rn(a4[a], b4[b]);
                    acc[a][b] = __dadd_rn(acc[a][b], __dmul_rn(df, df));
                }
        }
    }
}
