// kernels_graph.hip -- a graph view (include/cge_hip.h: cge_graph_view / cge_vertex_view) that lies in device memory, made into
// the resident tables: what parseargs does between `readdlm` and landmarks() (src/auxilary.jl:92-110, :133-139), on the device.
// gfx950, wave = 64.
//
//   extrema        : minimum and maximum id (only when the base or the vertex count is to be inferred, :92-99);
//   graph_ingest   : ids rebased, range-checked ON THE 64-BIT VALUE, narrowed to 0-based int32; the lowest bad edge by one 64-bit
//                    atomic min per workgroup; "some weight != 1.0" by one atomic OR per workgroup; fp32 weights widened (exact);
//   vertex_ingest  : community ids rebased and narrowed into comm / the padded uint16 table;
//   vertex_weights : vweight[u] += w; vweight[v] += w edge by edge (:107-110).  Unit weights: integer counts (exact in any order).
//                    Other weights: the sum is taken IN EDGE ORDER per vertex -- a stable sort of the 2 m (vertex, position) pairs
//                    gives every vertex its incident positions in file order, one lane walks a vertex's segment with a plain +=.
// No kernel here indexes by an id that has not passed the range check: graph_ingest only compares and stores ids, and the
// vertex_weights kernels run on the resident (validated) edge list.
#include "common.hpp"

namespace {
typedef long long ll;
struct IdI64 { typedef ll raw; };
struct IdI32 { typedef int raw; };
struct WNone {
    typedef double raw;
    static constexpr bool present = false;
};
struct WF64 {
    typedef double raw;
    static constexpr bool present = true;
};
struct WF32 {
    typedef float raw;
    static constexpr bool present = true;
};

// block-wide minimum / maximum of a 64-bit value (256 threads = 4 waves); every thread of the block must call it
__device__ __forceinline__ ll wave_min(ll v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const ll t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ ll wave_max(ll v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const ll t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}
} // namespace

// ---- extrema -----------------------------------------------------------------------------------------------------------------
// mm[0] = min, mm[1] = max over a[e * stride] (and b[e * stride] when b != NULL), e < count; mm starts at {INT64_MAX, INT64_MIN}
template <class I>
__global__ __launch_bounds__(256) void id_extrema_kernel(const typename I::raw *__restrict__ a, const typename I::raw *__restrict__ b,
                                                         i64 stride, i64 count, ll *__restrict__ mm) {
    __shared__ ll slo[4], shi[4];
    ll lo = INT64_MAX, hi = INT64_MIN;
    const i64 step = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += step) {
        const ll u = (ll)a[e * stride];
        lo = u < lo ? u : lo;
        hi = u > hi ? u : hi;
        if (b) {
            const ll v = (ll)b[e * stride];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) { lo = slo[k] < lo ? slo[k] : lo; hi = shi[k] > hi ? shi[k] : hi; }
        atomicMin(mm, lo);
        atomicMax(mm + 1, hi);
    }
}

// ---- graph_ingest ------------------------------------------------------------------------------------------------------------
// One slot = V edges.  MODE 0: element by element, any stride and alignment (a slice edge_index[:, 1:] is element-aligned and
// no more).  MODE 1: stride 1, both columns 16-byte aligned: one 16-byte load per column and slot (2 int64 / 4 int32 ids), the
// tail of m % V edges element by element.  MODE 2: an (m, 2) array (stride 2, dst = src + 1) with 16-byte aligned rows of pairs:
// one 16-byte load = one edge (int64) or two (int32).  Weights are read as they come (8 / 4 bytes per edge).
// flags[0] = lowest edge with an id outside [base, base + n) (starts at m), flags[1] |= 1 when some weight != 1.0.
template <class I, class W, int MODE>
__global__ __launch_bounds__(256) void graph_ingest_kernel(const typename I::raw *__restrict__ src, const typename I::raw *__restrict__ dst,
                                                           i64 stride, ll base, ll n, const typename W::raw *__restrict__ w, i64 m,
                                                           i32 *__restrict__ osrc, i32 *__restrict__ odst, double *__restrict__ ow,
                                                           ll *__restrict__ flags) {
    typedef typename I::raw raw;
    constexpr int V = MODE == 0 ? 1 : MODE == 1 ? 16 / (int)sizeof(raw) : 8 / (int)sizeof(raw);
    typedef raw rawv __attribute__((ext_vector_type(MODE == 0 ? 2 : 16 / (int)sizeof(raw))));
    __shared__ ll sbad[4];
    __shared__ int snon[4];
    ll bad = INT64_MAX;
    int non = 0;
    const i64 slots = (m + V - 1) / V, step = (i64)gridDim.x * blockDim.x;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < slots; q += step) {
        const i64 e0 = q * V;
        const int cnt = (int)(m - e0 < V ? m - e0 : V);
        ll u[V], v[V];
        if (MODE == 1 && cnt == V) {
            const rawv a = *(const rawv *)(src + e0), b = *(const rawv *)(dst + e0);
#pragma unroll
            for (int j = 0; j < V; j++) { u[j] = (ll)a[j]; v[j] = (ll)b[j]; }
        } else if (MODE == 2 && cnt == V) {
            const rawv a = *(const rawv *)(src + 2 * e0);
#pragma unroll
            for (int j = 0; j < V; j++) { u[j] = (ll)a[2 * j]; v[j] = (ll)a[2 * j + 1]; }
        } else {
#pragma unroll
            for (int j = 0; j < V; j++)
                if (j < cnt) { u[j] = (ll)src[(e0 + j) * stride]; v[j] = (ll)dst[(e0 + j) * stride]; }
        }
#pragma unroll
        for (int j = 0; j < V; j++)
            if (j < cnt) {
                // (unsigned: an id below the base wraps to a value >= 2^63 > n, so one comparison checks both ends)
                const unsigned long long a = (unsigned long long)u[j] - (unsigned long long)base,
                                         b = (unsigned long long)v[j] - (unsigned long long)base;
                if ((a >= (unsigned long long)n || b >= (unsigned long long)n) && e0 + j < bad) bad = e0 + j;
                osrc[e0 + j] = (i32)a;
                odst[e0 + j] = (i32)b;
                if (W::present) {
                    const double x = (double)w[e0 + j];
                    non |= x != 1.0;
                    ow[e0 + j] = x;
                }
            }
    }
    bad = wave_min(bad);
    non = __any(non) ? 1 : 0;
    if ((threadIdx.x & 63) == 0) { sbad[threadIdx.x >> 6] = bad; snon[threadIdx.x >> 6] = non; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) { bad = sbad[k] < bad ? sbad[k] : bad; non |= snon[k]; }
        if (bad != INT64_MAX) atomicMin(flags, bad);
        if (non) atomicOr((unsigned long long *)(flags + 1), 1ull);
    }
}

// ---- vertex_ingest -----------------------------------------------------------------------------------------------------------
// comm[i] = id - base (0-based; the caller has checked the extrema: base <= id, id - base < 2^31); comm16 likewise when given
template <class I>
__global__ __launch_bounds__(256) void vertex_ingest_kernel(const typename I::raw *__restrict__ ids, ll base, i64 n, i32 *__restrict__ comm,
                                                            unsigned short *__restrict__ comm16) {
    const i64 step = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const ll q = (ll)ids[i] - base;
        comm[i] = (i32)q;
        if (comm16) comm16[i] = (unsigned short)q;
    }
}

// ---- vertex_weights, unit weights ----------------------------------------------------------------------------------------------
// cnt[u]++, cnt[v]++ per edge (no-return 32-bit integer atomics on the n-entry table: exact in any order), then vw = (double)cnt
__global__ __launch_bounds__(256) void degree_count_kernel(const i32 *__restrict__ src, const i32 *__restrict__ dst, i64 m,
                                                           unsigned *__restrict__ cnt) {
    const i64 step = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += step) {
        atomicAdd(cnt + src[e], 1u);
        atomicAdd(cnt + dst[e], 1u);
    }
}
__global__ __launch_bounds__(256) void count_to_weight_kernel(const unsigned *__restrict__ cnt, i64 n, double *__restrict__ vw) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) vw[i] = (double)cnt[i];
}

// ---- vertex_weights, in edge order ---------------------------------------------------------------------------------------------
// the 2 m (vertex, position) pairs: position 2 e is edge e's source, 2 e + 1 its target (the order of the reference's two +=)
__global__ __launch_bounds__(256) void incidence_pairs_kernel(const i32 *__restrict__ src, const i32 *__restrict__ dst, i64 m,
                                                              unsigned *__restrict__ keys, i32 *__restrict__ pos) {
    const i64 step = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += step) {
        keys[2 * e] = (unsigned)src[e];
        keys[2 * e + 1] = (unsigned)dst[e];
        pos[2 * e] = (i32)(2 * e);
        pos[2 * e + 1] = (i32)(2 * e + 1);
    }
}
// seg[2 v], seg[2 v + 1] = the range of vertex v in the sorted pairs (seg starts zeroed: an isolated vertex keeps [0, 0))
__global__ __launch_bounds__(256) void segment_bounds_kernel(const unsigned *__restrict__ keys, i64 len, i32 *__restrict__ seg) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= len) return;
    const unsigned k = keys[j];
    if (j == 0 || keys[j - 1] != k) seg[2 * (i64)k] = (i32)j;
    if (j == len - 1 || keys[j + 1] != k) seg[2 * (i64)k + 1] = (i32)(j + 1);
}
// one lane per vertex: its incident weights in file order, added one after the other from 0.0 (a hub is one long chain by nature);
// the loads of eight terms are issued ahead of the adds that depend on them
__global__ __launch_bounds__(256) void ordered_sum_kernel(const i32 *__restrict__ seg, const i32 *__restrict__ pos,
                                                          const double *__restrict__ w, i64 n, double *__restrict__ vw) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const i32 a = seg[2 * v], b = seg[2 * v + 1];
    double s = 0.0;
    i32 j = a;
    for (; j + 8 <= b; j += 8) {
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = w[pos[j + k] >> 1];
#pragma unroll
        for (int k = 0; k < 8; k++) s += t[k];
    }
    for (; j < b; j++) s += w[pos[j] >> 1];
    vw[v] = s;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
void k_id_extrema(cge_ctx *c, const void *a, const void *b, i64 stride, int id_dtype, i64 count, i64 *d_minmax) {
    ScopedKernelTimer kt(c, "graph_extrema");
    const i64 init[2] = {INT64_MAX, INT64_MIN};
    HIP_CHECK(hipMemcpyAsync(d_minmax, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (`init` is on this frame)
    const unsigned grid = grid_for(count, 256, 4096);
    if (id_dtype == CGE_ID_I64)
        hipLaunchKernelGGL(id_extrema_kernel<IdI64>, dim3(grid), dim3(256), 0, c->stream, (const ll *)a, (const ll *)b, stride, count, (ll *)d_minmax);
    else
        hipLaunchKernelGGL(id_extrema_kernel<IdI32>, dim3(grid), dim3(256), 0, c->stream, (const int *)a, (const int *)b, stride, count, (ll *)d_minmax);
}

template <class I, class W>
static void launch_graph_ingest(cge_ctx *c, const void *src, const void *dst, i64 stride, i64 base, i64 n, const void *w, i64 m,
                                i32 *osrc, i32 *odst, double *ow, i64 *flags) {
    typedef typename I::raw raw;
    const raw *s = (const raw *)src, *d = (const raw *)dst;
    const typename W::raw *wp = (const typename W::raw *)w;
    const int mode = stride == 1 && (uintptr_t)s % 16 == 0 && (uintptr_t)d % 16 == 0 ? 1
                   : stride == 2 && d == s + 1 && (uintptr_t)s % 16 == 0             ? 2
                                                                                     : 0;
    const i64 V = mode == 0 ? 1 : mode == 1 ? 16 / (i64)sizeof(raw) : 8 / (i64)sizeof(raw);
    const unsigned grid = grid_for((m + V - 1) / V, 256, 1 << 16);
#define GI_LAUNCH(MODE) hipLaunchKernelGGL((graph_ingest_kernel<I, W, MODE>), dim3(grid), dim3(256), 0, c->stream, s, d, stride, (ll)base, (ll)n, wp, m, osrc, odst, ow, (ll *)flags)
    if (mode == 1) GI_LAUNCH(1);
    else if (mode == 2) GI_LAUNCH(2);
    else GI_LAUNCH(0);
#undef GI_LAUNCH
}
// flags (2 words on the device): [0] receives the lowest bad edge (m = none), [1] non-zero when some weight differs from 1.0
void k_graph_ingest(cge_ctx *c, const void *src, const void *dst, i64 stride, int id_dtype, i64 base, i64 n, const void *w, int w_dtype,
                    i64 m, i32 *osrc, i32 *odst, double *ow, i64 *flags) {
    ScopedKernelTimer kt(c, "graph_ingest");
    const i64 init[2] = {m, 0};
    HIP_CHECK(hipMemcpyAsync(flags, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (`init` is on this frame)
#define GI_W(I)                                                                                              \
    if (!w) launch_graph_ingest<I, WNone>(c, src, dst, stride, base, n, nullptr, m, osrc, odst, ow, flags);  \
    else if (w_dtype == CGE_DTYPE_F32) launch_graph_ingest<I, WF32>(c, src, dst, stride, base, n, w, m, osrc, odst, ow, flags); \
    else launch_graph_ingest<I, WF64>(c, src, dst, stride, base, n, w, m, osrc, odst, ow, flags)
    if (id_dtype == CGE_ID_I64) { GI_W(IdI64); }
    else { GI_W(IdI32); }
#undef GI_W
}

void k_vertex_ingest(cge_ctx *c, const void *ids, int id_dtype, i64 base, i64 n, i32 *comm, unsigned short *comm16) {
    ScopedKernelTimer kt(c, "vertex_ingest");
    const unsigned grid = grid_for(n, 256, 1 << 16);
    if (id_dtype == CGE_ID_I64)
        hipLaunchKernelGGL(vertex_ingest_kernel<IdI64>, dim3(grid), dim3(256), 0, c->stream, (const ll *)ids, (ll)base, n, comm, comm16);
    else
        hipLaunchKernelGGL(vertex_ingest_kernel<IdI32>, dim3(grid), dim3(256), 0, c->stream, (const int *)ids, (ll)base, n, comm, comm16);
}

void k_vertex_weights_unit(cge_ctx *c, const i32 *src, const i32 *dst, i64 m, i64 n, double *vw) {
    ScopedKernelTimer kt(c, "vertex_weights_unit");
    DevBuf<unsigned> cnt;
    cnt.alloc_exact((size_t)n);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned) * (size_t)n, c->stream));
    hipLaunchKernelGGL(degree_count_kernel, dim3(grid_for(m, 256, 1 << 16)), dim3(256), 0, c->stream, src, dst, m, cnt.p);
    hipLaunchKernelGGL(count_to_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, cnt.p, n, vw);
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (cnt goes out of scope)
}

// kernels_sort.hip: device-wide stable radix sort of (uint32 key, int32 value) pairs on the low `bits` bits
void k_sort_pairs_u32(cge_ctx *c, const unsigned *keys_in, unsigned *keys_out, const i32 *vals_in, i32 *vals_out, i64 n, int bits);

void k_vertex_weights_ordered(cge_ctx *c, const i32 *src, const i32 *dst, const double *w, i64 m, i64 n, double *vw) {
    ScopedKernelTimer kt(c, "vertex_weights_ordered");
    const i64 len = 2 * m;
    DevBuf<unsigned> keys, keys_s;
    DevBuf<i32> pos, pos_s, seg;
    keys.alloc_exact((size_t)len); keys_s.alloc_exact((size_t)len); pos.alloc_exact((size_t)len); pos_s.alloc_exact((size_t)len);
    seg.alloc_exact((size_t)(2 * n));
    HIP_CHECK(hipMemsetAsync(seg.p, 0, sizeof(i32) * (size_t)(2 * n), c->stream));
    hipLaunchKernelGGL(incidence_pairs_kernel, dim3(grid_for(m, 256, 1 << 16)), dim3(256), 0, c->stream, src, dst, m, keys.p, pos.p);
    int bits = 1;
    while (bits < 32 && ((i64)1 << bits) < n) bits++;
    k_sort_pairs_u32(c, keys.p, keys_s.p, pos.p, pos_s.p, len, bits); // (stable: equal vertices keep their positions ascending)
    hipLaunchKernelGGL(segment_bounds_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, keys_s.p, len, seg.p);
    hipLaunchKernelGGL(ordered_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, seg.p, pos_s.p, w, n, vw);
    HIP_CHECK(hipStreamSynchronize(c->stream)); // (the scratch buffers go out of scope)
}
