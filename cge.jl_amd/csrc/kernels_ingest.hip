// kernels_ingest.hip -- an embedding view (include/cge_hip.h: cge_embedding_view) of fp64 / fp32 / fp16 / bf16 elements, row- or
// column-major with a leading dimension, widened into the resident row-major fp64 matrix Xr.  gfx950, wave = 64.
//
// Widening is exact (every fp32 / fp16 / bf16 value, subnormals included, is an fp64 value), so Xr gets the bits of the caller's own
// `.astype(float64)` and nothing downstream can tell how the embedding came in.  The casts are plain C++: (double) of a float or a
// _Float16 keeps subnormals under hipcc's default denormal mode; a bf16 is the top half of a float.
//
// Three families, each templated on the source type:
//   rows   : row-major source -> Xr, a streaming convert (16-byte loads and stores per lane where the alignment allows);
//   cols   : column-major source (the whole matrix or an uploaded piece) -> Xr through LDS;
//   gather : listed rows of a device-resident source of either layout (option shard_rows).
// They are the library's only layout kernels: k_transpose_to_rowmajor and k_gather_rows_f64 at the end are the fp64 instances of
// cols and gather for scratch matrices.
#include "common.hpp"

namespace {
struct SrcF64 {
    typedef double raw;
    static __device__ __forceinline__ double widen(raw v) { return v; }
};
struct SrcF32 {
    typedef float raw;
    static __device__ __forceinline__ double widen(raw v) { return (double)v; }
};
struct SrcF16 {
    typedef _Float16 raw;
    static __device__ __forceinline__ double widen(raw v) { return (double)v; }
};
struct SrcBF16 {
    typedef unsigned short raw;
    static __device__ __forceinline__ double widen(raw v) { return (double)__uint_as_float((unsigned)v << 16); }
};
typedef double f64x2 __attribute__((ext_vector_type(2)));
} // namespace

// ---- rows --------------------------------------------------------------------------------------------------------------------
// dst[i * d + k] = src[i * ld + k].  A lane takes one 16-byte vector of a source row (2 / 4 / 8 elements) and writes it as 16-byte
// pairs of doubles; the last slot of a row is its tail of d % V elements, one by one.  The launcher hands a packed source over as
// ONE row of rows * d elements.  Needs: src and dst 16-byte aligned, and for rows > 1 a row pitch of whole vectors; with an odd d
// (rows > 1) the rows of dst are only 8-byte aligned and the stores go out as doubles (`pairs` = 0), the loads stay 16 bytes.
template <class S>
__global__ __launch_bounds__(256) void ingest_rows_vec_kernel(const typename S::raw *__restrict__ src, i64 ld, i64 rows, i64 d,
                                                              double *__restrict__ dst, int pairs) {
    typedef typename S::raw raw;
    constexpr int V = 16 / (int)sizeof(raw);
    typedef raw rawv __attribute__((ext_vector_type(V)));
    const i64 nv = d / V, per = nv + (d % V ? 1 : 0), total = rows * per, stride = (i64)gridDim.x * blockDim.x;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
        const i64 i = q / per, s = q - i * per;
        const raw *p = src + i * ld + s * V;
        double *o = dst + i * d + s * V;
        if (s < nv) {
            const rawv v = *(const rawv *)p;
#pragma unroll
            for (int j = 0; j < V; j += 2) {
                f64x2 w;
                w.x = S::widen(v[j]);
                w.y = S::widen(v[j + 1]);
                if (pairs) *(f64x2 *)(o + j) = w;
                else { o[j] = w.x; o[j + 1] = w.y; } // (an odd d: every other row of dst starts 8 bytes off)
            }
        } else {
            const int tail = (int)(d - nv * V);
            for (int j = 0; j < tail; j++) o[j] = S::widen(p[j]);
        }
    }
}
// the same, element by element: any alignment (a slice X[:, 1:] of a bf16 tensor is 2-byte aligned and no more), any d and ld
template <class S>
__global__ __launch_bounds__(256) void ingest_rows_kernel(const typename S::raw *__restrict__ src, i64 ld, i64 rows, i64 d,
                                                          double *__restrict__ dst) {
    const i64 total = rows * d, stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const i64 i = e / d, k = e - i * d;
        dst[e] = S::widen(src[i * ld + k]);
    }
}

// ---- cols --------------------------------------------------------------------------------------------------------------------
// Rows [i0, i0 + rows) x columns [k0, k0 + cols) of Xr (row pitch d) from a column-major piece src[k * ld + i].  A tile is 64 rows
// x 32 columns: the read takes 64 consecutive elements of a source column per row of lanes (128 B of a 2-byte type, 512 B of
// fp64), the write 32 consecutive doubles of a row of Xr (256 B).  The tile holds doubles (widened on the way in); its pitch of 65
// keeps both sides off each other's LDS banks (the read-back walks a column of the tile: 130 dwords from lane to lane).
template <class S>
__global__ __launch_bounds__(256) void ingest_cols_kernel(const typename S::raw *__restrict__ src, i64 ld, double *__restrict__ Xrow,
                                                          i64 rows, i64 cols, i64 i0, i64 k0, i64 d) {
    __shared__ double tile[32][65];
    const i64 ib = (i64)blockIdx.x * 64, kb = (i64)blockIdx.y * 32;
    const int t = threadIdx.x;
    {
        const int tx = t & 63, ty = t >> 6; // 64 x 4
        const i64 i = ib + tx;
        for (int r = ty; r < 32; r += 4) {
            const i64 k = kb + r;
            if (i < rows && k < cols) tile[r][tx] = S::widen(src[k * ld + i]);
        }
    }
    __syncthreads();
    {
        const int tx = t & 31, ty = t >> 5; // 32 x 8
        const i64 k = kb + tx;
        for (int r = ty; r < 64; r += 8) {
            const i64 i = ib + r;
            if (i < rows && k < cols) Xrow[(i0 + i) * d + k0 + k] = tile[tx][r];
        }
    }
}

// ---- gather ------------------------------------------------------------------------------------------------------------------
// out[i][k] = X[idx[i]][k] of a row-major (X[g * ld + k]) or column-major (X[k * ld + g]) source; a negative index: a zero row
template <class S>
__global__ __launch_bounds__(256) void ingest_gather_kernel(const typename S::raw *__restrict__ X, i64 ld, i64 d, int row_major,
                                                            const i32 *__restrict__ idx, i64 cnt, double *__restrict__ out) {
    const i64 total = cnt * d, stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const i64 i = e / d, k = e - i * d, g = idx[i];
        out[e] = g < 0 ? 0.0 : S::widen(row_major ? X[g * ld + k] : X[k * ld + g]);
    }
}

// ---- launchers (dtype: CGE_DTYPE_*, checked at the boundary) -----------------------------------------------------------------
#define INGEST_DISPATCH(dtype, CALL)            \
    switch (dtype) {                            \
    case CGE_DTYPE_F64: { typedef SrcF64 S; CALL; } break;  \
    case CGE_DTYPE_F32: { typedef SrcF32 S; CALL; } break;  \
    case CGE_DTYPE_F16: { typedef SrcF16 S; CALL; } break;  \
    case CGE_DTYPE_BF16: { typedef SrcBF16 S; CALL; } break; \
    default: CGE_THROW(CGE_E_ARG, "embedding view: unknown dtype %d", (int)(dtype)); \
    }

size_t cge_dtype_size(int dtype) { return dtype == CGE_DTYPE_F64 ? 8 : dtype == CGE_DTYPE_F32 ? 4 : 2; }

void k_ingest_rows(cge_ctx *c, const void *src, int dtype, i64 ld, i64 rows, i64 d, double *dst) {
    if (rows <= 0 || d <= 0) return;
    ScopedKernelTimer kt(c, "ingest_rows");
    if (ld == d) { d *= rows; ld = d; rows = 1; } // packed: one long row
    const size_t es = cge_dtype_size(dtype);
    const i64 V = (i64)(16 / es);
    const bool vec = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && (rows == 1 || (size_t)ld * es % 16 == 0);
    if (vec) {
        const unsigned grid = grid_for(rows * ((d + V - 1) / V), 256, 1 << 16);
        INGEST_DISPATCH(dtype, hipLaunchKernelGGL(ingest_rows_vec_kernel<S>, dim3(grid), dim3(256), 0, c->stream,
                                                  (const S::raw *)src, ld, rows, d, dst, (int)(rows == 1 || d % 2 == 0)));
    } else {
        const unsigned grid = grid_for(rows * d, 256, 1 << 16);
        INGEST_DISPATCH(dtype, hipLaunchKernelGGL(ingest_rows_kernel<S>, dim3(grid), dim3(256), 0, c->stream, (const S::raw *)src,
                                                  ld, rows, d, dst));
    }
}
static void launch_cols(cge_ctx *c, const void *src, int dtype, i64 ld, double *Xrow, i64 rows, i64 cols, i64 i0, i64 k0, i64 d) {
    const size_t es = cge_dtype_size(dtype);
    const i64 kmax = (i64)65535 * 32; // columns of one launch (grid.y)
    for (i64 ka = 0; ka < cols; ka += kmax) {
        const i64 kc = std::min(kmax, cols - ka);
        const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((kc + 31) / 32));
        const void *p = (const unsigned char *)src + (size_t)ka * (size_t)ld * es;
        INGEST_DISPATCH(dtype, hipLaunchKernelGGL(ingest_cols_kernel<S>, grid, dim3(256), 0, c->stream, (const S::raw *)p, ld, Xrow,
                                                  rows, kc, i0, k0 + ka, d));
    }
}
static void launch_gather(cge_ctx *c, const void *X, int dtype, i64 ld, i64 d, int row_major, const i32 *idx, i64 cnt, double *out) {
    INGEST_DISPATCH(dtype, hipLaunchKernelGGL(ingest_gather_kernel<S>, dim3(grid_for(cnt * d, 256, 8192)), dim3(256), 0, c->stream,
                                              (const S::raw *)X, ld, d, row_major, idx, cnt, out));
}
void k_ingest_cols(cge_ctx *c, const void *src, int dtype, i64 ld, double *Xrow, i64 rows, i64 cols, i64 i0, i64 k0, i64 d) {
    if (rows <= 0 || cols <= 0) return;
    ScopedKernelTimer kt(c, "ingest_cols");
    launch_cols(c, src, dtype, ld, Xrow, rows, cols, i0, k0, d);
}
void k_ingest_gather(cge_ctx *c, const void *X, int dtype, i64 ld, i64 d, int row_major, const i32 *idx, i64 cnt, double *out) {
    if (cnt <= 0 || d <= 0) return;
    ScopedKernelTimer kt(c, "ingest_gather");
    launch_gather(c, X, dtype, ld, d, row_major, idx, cnt, out);
}
// packed fp64 scratch matrices, no timer (common.hpp): a column-major n x d matrix -> row-major; listed rows of an n x d matrix
void k_transpose_to_rowmajor(cge_ctx *c, const double *Xcol, double *Xrow, i64 n, i64 d) {
    if (n > 0 && d > 0) launch_cols(c, Xcol, CGE_DTYPE_F64, n, Xrow, n, d, 0, 0, d);
}
void k_gather_rows_f64(cge_ctx *c, const double *X, i64 n, i64 d, int row_major, const i32 *idx, i64 cnt, double *out) {
    if (cnt > 0 && d > 0) launch_gather(c, X, CGE_DTYPE_F64, row_major ? d : n, d, row_major, idx, cnt, out);
}
