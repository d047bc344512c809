// link_p.hpp -- the ONE definition of the link model's probability, shared by the kernels that must agree with cge_link_prob bit
// for bit (kernels_link.hip: per pair; kernels_linktri.hip: the matrix Q tile by tile).  gfx950 only.
//
//     p(i, j) = (f_out[i] * f_in[j]) * max(0, 1 - dist(i, j) / hi) ^ alpha
#pragma once
#include "common.hpp"
#include "pow_parts.hpp"

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
// the value from a distance already summed in link_dist's order (a tile loop that adds the same terms: dist_tile.hpp)
template <bool EXP2>
__device__ __forceinline__ double link_p_dist(double dist, double fo, double fi, double hi, double alpha) {
    const double x = dist / hi;
    return (fo * fi) * link_power<EXP2>(x, alpha);
}
template <bool EXP2>
__device__ __forceinline__ double link_p(const double *__restrict__ Xr, i64 d, i64 i, i64 j, double fo, double fi, double hi,
                                         double alpha) {
    return link_p_dist<EXP2>(link_dist(Xr, d, i, j), fo, fi, hi, alpha);
}

__device__ __forceinline__ void lds_sync() { // (the LDS stores of this wave have landed before the barrier: tests/test_device_asm.py)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}
