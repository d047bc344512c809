// kernels_louvain.hip -- Louvain on the resident graph: level 1 is the communities `louvain_clust` writes to <file>.ecg
// when the command line has no `-c` (src/clustering.jl:14-68, src/auxilary.jl:115-121); the further
// levels (the reference's executable computes them all, `louvain -l -1`, and `hierarchy -l 1` throws them away,
// src/clustering.jl:20-24) are the same pass on the graph contracted by the level before (k_louvain_levels, below).
//
// The reference shells out to the "generic Louvain" executables (convert / louvain -l -1 -q 0 / hierarchy -l 1): the
// partition after the FIRST pass of local moving, nodes visited one at a time in a rand()-shuffled order.  On the GPU the
// pass is synchronous: in every round each vertex looks at the communities of its neighbours as they stood at the start
// of the round (its adjacency segment sorted by community: a segmented radix sort, so the sums over a community are
// contiguous runs and the choice is deterministic), takes the one of largest gain  k_vc - tot_c k_v / 2m  (its own
// community first, so ties stay; the smallest id among equal gains otherwise), and all moves are applied together.  Two
// guards keep simultaneous moves from chasing each other: two singletons only merge towards the smaller id, and a vertex
// may only move in every other round (by a hash of its id).  The host keeps the best partition seen (synchronous rounds
// are not monotone in the modularity) and stops after three rounds without an improvement of more than 1e-6 (the
// reference's own threshold) or when nothing WANTS to move: no vertex has a strictly better community that the singleton
// guard allows.  A vertex that the turn guard alone holds back keeps the pass going (its turn is the next round), so a round
// in which nothing moved is not the end by itself.  When every edge is a self loop there is nothing to move and the
// singleton partition is returned with its own modularity (a self loop counts once in k_v and once in "in").
// Not bit-comparable with the reference (whose visiting order is random): tests compare modularity and structure with the
// sequential restatement in the oracle and with networkx, and the rounds themselves -- partition, round count, modularity
// -- with the numpy restatement tests/louvain_ref.py, exactly on integer and dyadic weights (-ffp-contract=off: the sums
// are exact there, whatever their order).
//
// A pass runs on a CSR graph (off, adj, aw, self, n).  Level 1's is filled from the resident edge list through atomic cursors;
// level L + 1's is the contraction of level L's by its renumbered partition (`partition2graph_binary` of generic Louvain): the
// coarse vertices are the communities, entry (C, D), C != D, is the sum of the fine entries (v in C, u in D) -- repeated edges
// merge, the coarse adjacency is always weighted -- and self[C] = sum_{v in C} self[v] + the fine entries with both ends in C
// (an inner edge is seen from both ends and counts twice, an original self loop once).  So k_C = tot_C, m2 is unchanged and the
// coarse singletons have the modularity of the fine partition.  One (C, D) key and a weight per entry (and per vertex: its self
// loop under (C, C)), one stable device-wide radix sort, head flags, one integer scan, and each run summed by plain += in
// ascending sorted position: no float atomics, no reduce_by_key (a decoupled look-back does not fix the order of additions).
//
// Exactness: on integer and dyadic weights every sum is exact in any order, so partitions, community counts, round counts and
// modularities of EVERY level are determined to the bit and equal tests/louvain_levels_ref.py.  On other weights only the
// quality is comparable, and results may differ between runs, as level 1's already can (its adjacency is filled through atomic
// cursors, so the order of a segment -- and of the entries of a coarse run -- is not fixed).
#include "common.hpp"

#include <rocprim/rocprim.hpp>

__global__ void lv_count_kernel(const i32 *__restrict__ src, const i32 *__restrict__ dst, i64 m, i32 *__restrict__ cnt) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const i32 u = src[e], v = dst[e];
        if (u == v) continue; // self loops are kept aside (lv_fill_kernel)
        atomicAdd(&cnt[u], 1);
        atomicAdd(&cnt[v], 1);
    }
}
__global__ void lv_fill_kernel(const i32 *__restrict__ src, const i32 *__restrict__ dst, const double *__restrict__ w, i64 m,
                               const i32 *__restrict__ off, i32 *__restrict__ cur, i32 *__restrict__ adj,
                               double *__restrict__ aw, double *__restrict__ self) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const i32 u = src[e], v = dst[e];
        const double we = w ? w[e] : 1.0;
        if (u == v) { unsafeAtomicAdd(&self[u], we); continue; }
        const i32 pu = off[u] + atomicAdd(&cur[u], 1), pv = off[v] + atomicAdd(&cur[v], 1);
        adj[pu] = v; adj[pv] = u;
        if (aw) { aw[pu] = we; aw[pv] = we; }
    }
}
// weighted degree k_v (self loop counted once, as `convert` stores it), tot_c = k_v for the singleton start
__global__ void lv_degree_kernel(const i32 *__restrict__ off, const double *__restrict__ aw, const double *__restrict__ self,
                                 i64 n, double *__restrict__ k, double *__restrict__ tot, i32 *__restrict__ comm,
                                 i32 *__restrict__ size, double *__restrict__ m2) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    double kv = 0.0;
    if (v < n) {
        if (aw) for (i32 q = off[v]; q < off[v + 1]; q++) kv += aw[q];
        else kv = (double)(off[v + 1] - off[v]);
        kv += self[v];
        k[v] = kv;
        tot[v] = kv;
        comm[v] = (i32)v;
        size[v] = 1;
    }
    for (int o = 32; o > 0; o >>= 1) kv += __shfl_down(kv, o);
    if ((threadIdx.x & 63) == 0 && kv != 0.0) unsafeAtomicAdd(m2, kv);
}
__global__ void lv_keys_kernel(const i32 *__restrict__ adj, const i32 *__restrict__ comm, i64 len, unsigned *__restrict__ keys) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < len; q += stride) keys[q] = (unsigned)comm[adj[q]];
}
// one thread per vertex: the runs of its community-sorted adjacency segment -> the community of largest gain.
// stats[0] += moves, stats[1] += sum_v (k_{v,own} + self_v)  (the "in" part of the modularity of the CURRENT partition),
// stats[3] += vertices that want to move: a strictly better community that the singleton guard allows, on turn or not
// SKIP (levels >= 2): a vertex whose segment is longer than `ell` is left to lv_decide_wave_kernel
template <bool SKIP>
__global__ void lv_decide_kernel(const i32 *__restrict__ off, const unsigned *__restrict__ skeys, const double *__restrict__ saw,
                                 const double *__restrict__ self, const double *__restrict__ k, const double *__restrict__ tot,
                                 const i32 *__restrict__ size, const i32 *__restrict__ comm, i64 n, double m2, int round,
                                 i32 *__restrict__ newcomm, double *__restrict__ stats, i32 ell) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    double in_part = 0.0, moved = 0.0, wants = 0.0;
    if (v < n && !(SKIP && off[v + 1] - off[v] > ell)) {
        const i32 own = comm[v];
        const double kv = k[v];
        // pass 1: weight towards the own community
        double w_own = 0.0;
        for (i32 q = off[v]; q < off[v + 1]; q++)
            if ((i32)skeys[q] == own) w_own += saw ? saw[q] : 1.0;
        in_part = w_own + self[v];
        i32 best = own;
        double best_inc = w_own - (tot[own] - kv) * kv / m2;
        // pass 2: the other communities, ascending id (the segment is sorted), strict improvement only
        i32 q = off[v];
        const i32 qe = off[v + 1];
        while (q < qe) {
            const i32 c = (i32)skeys[q];
            double ws = 0.0;
            while (q < qe && (i32)skeys[q] == c) { ws += saw ? saw[q] : 1.0; q++; }
            if (c == own) continue;
            const double inc = ws - tot[c] * kv / m2;
            if (inc > best_inc) { best = c; best_inc = inc; }
        }
        const bool my_turn = ((((unsigned)v * 2654435761u) >> 15) & 1u) == (unsigned)(round & 1);
        if (best != own && size[own] == 1 && size[best] == 1 && best > own) best = own;
        wants = best != own ? 1.0 : 0.0;
        if (!my_turn) best = own;
        newcomm[v] = best;
        moved = best != own ? 1.0 : 0.0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        in_part += __shfl_down(in_part, o);
        moved += __shfl_down(moved, o);
        wants += __shfl_down(wants, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (moved != 0.0) unsafeAtomicAdd(&stats[0], moved);
        if (wants != 0.0) unsafeAtomicAdd(&stats[3], wants);
        if (in_part != 0.0) unsafeAtomicAdd(&stats[1], in_part);
    }
}
__global__ void lv_apply_kernel(i32 *__restrict__ comm, const i32 *__restrict__ newcomm, const double *__restrict__ k, i64 n,
                                double *__restrict__ tot, i32 *__restrict__ size) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const i32 a = comm[v], b = newcomm[v];
    if (a == b) return;
    unsafeAtomicAdd(&tot[a], -k[v]);
    unsafeAtomicAdd(&tot[b], k[v]);
    atomicAdd(&size[a], -1);
    atomicAdd(&size[b], 1);
    comm[v] = b;
}
// stats[2] += sum_c tot_c^2 over the non-empty communities
__global__ void lv_totsq_kernel(const double *__restrict__ tot, const i32 *__restrict__ size, i64 n, double *__restrict__ stats) {
    const i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    double s = (c < n && size[c] > 0) ? tot[c] * tot[c] : 0.0;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0 && s != 0.0) unsafeAtomicAdd(&stats[2], s);
}
__global__ void lv_used_kernel(const i32 *__restrict__ comm, i64 n, i32 *__restrict__ used) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) used[comm[v]] = 1;
}
__global__ void lv_renumber_kernel(const i32 *__restrict__ comm, const i32 *__restrict__ newid, i64 n, i64 *__restrict__ out) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) out[v] = newid[comm[v]];
}


// ---- levels >= 2: the decision of a long segment by one wave ------------------------------------------------------------------
// A coarse vertex can have thousands of neighbours, and in lv_decide_kernel the other 63 lanes of its wave wait for it.
__global__ void lv_long_kernel(const i32 *__restrict__ off, i64 n, i32 ell, i32 *__restrict__ list, i32 *__restrict__ cnt) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && off[v + 1] - off[v] > ell) list[atomicAdd(cnt, 1)] = (i32)v;
}
// one wave per listed vertex, the same decision as the lane form and the same `stats` words: w_own by a strided sum and a wave
// reduction; the runs of the community-sorted segment by a segmented scan over 64-entry chunks, the run that crosses a chunk
// boundary carried in (carry_c, carry_ws); the winner by a wave arg-max under the lane form's rule (the own community wins ties,
// otherwise the smallest id among equal gains), then the singleton guard and the turn bit.  The sums are taken in another order
// than the lane form's: the same bits on integer and dyadic weights
__global__ __launch_bounds__(256) void lv_decide_wave_kernel(const i32 *__restrict__ list, i32 nlist, const i32 *__restrict__ off,
                                                             const unsigned *__restrict__ skeys, const double *__restrict__ saw,
                                                             const double *__restrict__ self, const double *__restrict__ k,
                                                             const double *__restrict__ tot, const i32 *__restrict__ size,
                                                             const i32 *__restrict__ comm, double m2, int round,
                                                             i32 *__restrict__ newcomm, double *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    double in_part = 0.0, moved = 0.0, wants = 0.0; // lane 0's
    for (i64 i = wave; i < nlist; i += nwaves) {
        const i32 v = list[i];
        const i32 own = comm[v];
        const double kv = k[v];
        const i32 a = off[v], b = off[v + 1];
        double w_own = 0.0;
        for (i32 q = a + lane; q < b; q += 64)
            if ((i32)skeys[q] == own) w_own += saw[q];
        for (int o = 32; o > 0; o >>= 1) w_own += __shfl_xor(w_own, o);
        // this lane's best among the other communities (it meets them in ascending id)
        i32 best = INT32_MAX;
        double best_inc = -INFINITY;
        i32 carry_c = -1;
        double carry_ws = 0.0;
        for (i32 base = a; base < b; base += 64) {
            const i32 q = base + lane;
            const bool valid = q < b;
            const i32 c = valid ? (i32)skeys[q] : -2;
            const i32 cn = (valid && q + 1 < b) ? (i32)skeys[q + 1] : -2;
            double ws = valid ? saw[q] : 0.0;
            for (int d = 1; d < 64; d <<= 1) { // (sorted keys: equal ends mean an equal stretch)
                const double t = __shfl_up(ws, d);
                const i32 cu = __shfl_up(c, d);
                if (lane >= d && cu == c) ws += t;
            }
            if (c == carry_c) ws += carry_ws;
            if (valid && cn != c && c != own) { // the run ends here
                const double inc = ws - tot[c] * kv / m2;
                if (inc > best_inc) { best = c; best_inc = inc; }
            }
            carry_c = __shfl(c, 63);
            carry_ws = __shfl(ws, 63);
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double oi = __shfl_xor(best_inc, o);
            const i32 oc = __shfl_xor(best, o);
            if (oi > best_inc || (oi == best_inc && oc < best)) { best = oc; best_inc = oi; }
        }
        if (lane == 0) {
            i32 pick = best_inc > w_own - (tot[own] - kv) * kv / m2 ? best : own;
            const bool my_turn = ((((unsigned)v * 2654435761u) >> 15) & 1u) == (unsigned)(round & 1);
            if (pick != own && size[own] == 1 && size[pick] == 1 && pick > own) pick = own;
            wants += pick != own ? 1.0 : 0.0;
            if (!my_turn) pick = own;
            newcomm[v] = pick;
            moved += pick != own ? 1.0 : 0.0;
            in_part += w_own + self[v];
        }
    }
    if (lane == 0) {
        if (moved != 0.0) unsafeAtomicAdd(&stats[0], moved);
        if (wants != 0.0) unsafeAtomicAdd(&stats[3], wants);
        if (in_part != 0.0) unsafeAtomicAdd(&stats[1], in_part);
    }
}

// ---- the contraction of a level's graph by its renumbered partition --------------------------------------------------------------
// entry j < len of vertex v (found by bisection of off): key (comm[v] << cb | comm[adj[j]]) and its weight; entry len + v: the
// self loop of vertex v under (comm[v], comm[v]) -- so every coarse vertex has a (C, C) run, whatever its inner edges
__global__ void lv_ckeys_kernel(const i32 *__restrict__ off, const i32 *__restrict__ adj, const double *__restrict__ aw,
                                const double *__restrict__ self, const i64 *__restrict__ comm, i64 n, i64 len, int cb,
                                unsigned long long *__restrict__ keys, double *__restrict__ vals) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < len + n; j += stride) {
        i64 C, D;
        double w;
        if (j < len) {
            i64 lo = 0, hi = n; // off[lo] <= j, and hi == n or off[hi] > j
            while (hi - lo > 1) {
                const i64 mid = (lo + hi) >> 1;
                if (off[mid] <= j) lo = mid; else hi = mid;
            }
            C = comm[lo];
            D = comm[adj[j]];
            w = aw ? aw[j] : 1.0;
        } else {
            C = D = comm[j - len];
            w = self[j - len];
        }
        keys[j] = ((unsigned long long)C << cb) | (unsigned long long)D;
        vals[j] = w;
    }
}
// flag[j] = 1 where a run of equal keys starts (j < total), flag[total] = 0: its exclusive scan numbers the runs and counts them
__global__ void lv_heads_kernel(const unsigned long long *__restrict__ skeys, i64 total, i32 *__restrict__ flag) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= total) flag[j] = j < total && (j == 0 || skeys[j] != skeys[j - 1]) ? 1 : 0;
}
__global__ void lv_starts_kernel(const unsigned long long *__restrict__ skeys, const i32 *__restrict__ ridx, i64 total,
                                 i32 *__restrict__ start) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    if (j == 0 || skeys[j] != skeys[j - 1]) start[ridx[j]] = (i32)j;
    if (j == 0) start[ridx[total]] = (i32)total;
}
// one lane per run r of the sorted entries: its weights added one after the other, in ascending sorted position, from 0.0; the
// loads of eight terms go ahead of the adds that depend on them.  A run of more than 64 entries is then taken by the whole wave:
// 64 coalesced loads (the next chunk's issued before this chunk's adds), and the same chain of adds in every lane.  Row C's runs
// are its (C, C) run and its coarse neighbours in ascending id, and rows 0 .. C-1 have one (C', C') run each, so the run lands at
// adjacency position r - C - (D > C), and row C starts at (its first run) - C
__global__ __launch_bounds__(256) void lv_runsum_kernel(const unsigned long long *__restrict__ skeys, const double *__restrict__ svals,
                                                        const i32 *__restrict__ start, i64 R, i64 nc, int cb, i32 *__restrict__ off2,
                                                        i32 *__restrict__ adj2, double *__restrict__ aw2, double *__restrict__ self2) {
    const i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const i32 a = r < R ? start[r] : 0, b = r < R ? start[r + 1] : 0;
    double s = 0.0;
    if (b - a <= 64) {
        i32 j = a;
        for (; j + 8 <= b; j += 8) {
            double t[8];
#pragma unroll
            for (int q = 0; q < 8; q++) t[q] = svals[j + q];
#pragma unroll
            for (int q = 0; q < 8; q++) s += t[q];
        }
        for (; j < b; j++) s += svals[j];
    }
    unsigned long long longs = __ballot(b - a > 64);
    while (longs) {
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const i32 wa = __shfl(a, src), wb = __shfl(b, src);
        double ws = 0.0, t = wa + lane < wb ? svals[wa + lane] : 0.0;
        for (i32 base = wa; base < wb; base += 64) {
            const double tn = base + 64 + lane < wb ? svals[base + 64 + lane] : 0.0;
#pragma unroll
            for (int q = 0; q < 64; q++) ws += __shfl(t, q); // (the padding of the last chunk adds 0.0)
            t = tn;
        }
        if (lane == src) s = ws;
    }
    if (r >= R) return;
    const unsigned long long key = skeys[a];
    const i64 C = (i64)(key >> cb), D = (i64)(key & ((1ull << cb) - 1));
    if (a == 0 || (i64)(skeys[a - 1] >> cb) != C) off2[C] = (i32)(r - C);
    if (r == R - 1) off2[nc] = (i32)(R - nc);
    if (C == D) self2[C] = s;
    else {
        const i64 p = r - C - (D > C ? 1 : 0);
        adj2[p] = (i32)D;
        aw2[p] = s;
    }
}
__global__ void lv_compose_kernel(i64 *__restrict__ comp, const i64 *__restrict__ lvl, i64 n) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) comp[v] = lvl[comp[v]];
}

#define LV_WAVE_LEN 128 // levels >= 2: segments longer than this are decided by a wave (DESIGN 7d has the measurement)

struct LvGraph { // every edge both ways in adj / aw (aw empty: unit weights), self loops aside
    DevBuf<i32> off, adj;
    DevBuf<double> aw, self;
    i64 n = 0, len = 0;
    bool weighted = false;
};

// level 1's graph, from the resident edge list
static void lv_build_csr(cge_ctx *c, LvGraph &g) {
    const i64 n = c->n, m = c->m;
    hipStream_t st = c->stream;
    DevBuf<i32> cur;
    g.n = n;
    g.off.ensure(n + 1); cur.ensure(n);
    HIP_CHECK(hipMemsetAsync(g.off.p, 0, sizeof(i32) * (n + 1), st));
    HIP_CHECK(hipMemsetAsync(cur.p, 0, sizeof(i32) * n, st));
    hipLaunchKernelGGL(lv_count_kernel, dim3(grid_for(m, 256)), dim3(256), 0, st, c->src.p, c->dst.p, m, g.off.p + 1);
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::inclusive_scan(nullptr, bytes, g.off.p, g.off.p, (size_t)(n + 1), rocprim::plus<i32>(), st));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::inclusive_scan(c->sort_tmp.p, bytes, g.off.p, g.off.p, (size_t)(n + 1), rocprim::plus<i32>(), st));
    }
    i32 len32 = 0;
    HIP_CHECK(hipMemcpyAsync(&len32, g.off.p + n, sizeof(i32), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    g.len = len32;
    g.weighted = !c->unit_weights;
    g.adj.ensure(g.len);
    if (g.weighted) g.aw.ensure(g.len);
    g.self.ensure(n);
    HIP_CHECK(hipMemsetAsync(g.self.p, 0, sizeof(double) * n, st));
    hipLaunchKernelGGL(lv_fill_kernel, dim3(grid_for(m, 256)), dim3(256), 0, st, c->src.p, c->dst.p, g.weighted ? c->w.p : nullptr, m,
                       g.off.p, cur.p, g.adj.p, g.weighted ? g.aw.p : nullptr, g.self.p);
    HIP_CHECK(hipStreamSynchronize(st)); // (`cur` goes with this frame)
}

// one pass of local moving on g: out[v] in 0 .. *n_comm-1 on the device (ascending order of the old community ids, as the
// reference's renumbering), *quality = modularity of the returned partition, *rounds_out = synchronous rounds run.  Level 1
// decides every vertex in a lane; from level 2 on the segments longer than `ell` go to lv_decide_wave_kernel
static void lv_pass(cge_ctx *c, const LvGraph &g, int level, DevBuf<i64> &out, i64 *n_comm, double *quality, i64 *rounds_out) {
    const i64 n = g.n, len = g.len;
    const bool weighted = g.weighted;
    hipStream_t st = c->stream;
    const unsigned gv = (unsigned)((n + 255) / 256);
    DevBuf<i32> comm, newcomm, size, best, used, newid, longs, nlong_d;
    DevBuf<unsigned> keys, skeys;
    DevBuf<double> saw, k, tot, stats;
    const double *aw = weighted ? g.aw.p : nullptr;
    keys.ensure(len); skeys.ensure(len);
    if (weighted) saw.ensure(len);
    k.ensure(n); tot.ensure(n); comm.ensure(n); newcomm.ensure(n); size.ensure(n); best.ensure(n);
    stats.ensure(5); // moves, in, sum tot^2, wants (cleared every round); m2
    HIP_CHECK(hipMemsetAsync(stats.p, 0, sizeof(double) * 5, st));
    hipLaunchKernelGGL(lv_degree_kernel, dim3(gv), dim3(256), 0, st, g.off.p, aw, g.self.p, n, k.p, tot.p, comm.p, size.p, stats.p + 4);
    double hs[5];
    HIP_CHECK(hipMemcpyAsync(hs, stats.p, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const double m2 = hs[4];
    int bits = 1;
    while (((i64)1 << bits) < n) bits++;
    // the wave form's list (once per level)
    const i64 knob = c->opt_test_louvain_wave_len; // -2: the default, -1: every vertex, >= 0: segments longer than this (2^31 - 1: none)
    const i32 ell = knob == -2 ? LV_WAVE_LEN : (i32)knob;
    i32 nlong = 0;
    const bool split = level >= 2 && weighted && ell < INT32_MAX && m2 > 0.0 && len > 0;
    if (split) {
        longs.ensure(n); nlong_d.ensure(1);
        HIP_CHECK(hipMemsetAsync(nlong_d.p, 0, sizeof(i32), st));
        hipLaunchKernelGGL(lv_long_kernel, dim3(gv), dim3(256), 0, st, g.off.p, n, ell, longs.p, nlong_d.p);
        HIP_CHECK(hipMemcpyAsync(&nlong, nlong_d.p, sizeof(i32), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    double best_q = -1e300;
    int since_best = 0;
    i64 rounds = 0;
    if (m2 > 0.0 && len > 0) {
        for (int round = 0; round < 200; round++) {
            rounds = round + 1;
            hipLaunchKernelGGL(lv_keys_kernel, dim3(grid_for(len, 256)), dim3(256), 0, st, g.adj.p, comm.p, len, keys.p);
            size_t bytes = 0;
            if (weighted) {
                HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, bytes, keys.p, skeys.p, aw, saw.p, (unsigned)len, (unsigned)n,
                                                              g.off.p, g.off.p + 1, 0, bits, st));
                c->sort_tmp.ensure(bytes);
                HIP_CHECK(rocprim::segmented_radix_sort_pairs(c->sort_tmp.p, bytes, keys.p, skeys.p, aw, saw.p, (unsigned)len,
                                                              (unsigned)n, g.off.p, g.off.p + 1, 0, bits, st));
            } else {
                HIP_CHECK(rocprim::segmented_radix_sort_keys(nullptr, bytes, keys.p, skeys.p, (unsigned)len, (unsigned)n, g.off.p,
                                                             g.off.p + 1, 0, bits, st));
                c->sort_tmp.ensure(bytes);
                HIP_CHECK(rocprim::segmented_radix_sort_keys(c->sort_tmp.p, bytes, keys.p, skeys.p, (unsigned)len, (unsigned)n, g.off.p,
                                                             g.off.p + 1, 0, bits, st));
            }
            HIP_CHECK(hipMemsetAsync(stats.p, 0, sizeof(double) * 4, st));
            if (nlong > 0) {
                hipLaunchKernelGGL(lv_decide_kernel<true>, dim3(gv), dim3(256), 0, st, g.off.p, skeys.p, saw.p, g.self.p, k.p, tot.p,
                                   size.p, comm.p, n, m2, round, newcomm.p, stats.p, ell);
                hipLaunchKernelGGL(lv_decide_wave_kernel, dim3(grid_for(nlong, 4)), dim3(256), 0, st, longs.p, nlong, g.off.p, skeys.p,
                                   saw.p, g.self.p, k.p, tot.p, size.p, comm.p, m2, round, newcomm.p, stats.p);
            } else
                hipLaunchKernelGGL(lv_decide_kernel<false>, dim3(gv), dim3(256), 0, st, g.off.p, skeys.p, weighted ? saw.p : nullptr,
                                   g.self.p, k.p, tot.p, size.p, comm.p, n, m2, round, newcomm.p, stats.p, 0);
            hipLaunchKernelGGL(lv_totsq_kernel, dim3(gv), dim3(256), 0, st, tot.p, size.p, n, stats.p);
            HIP_CHECK(hipMemcpyAsync(hs, stats.p, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            const double q = hs[1] / m2 - hs[2] / (m2 * m2); // modularity of the partition this round STARTED from
            if (q > best_q + 1e-6) {
                best_q = q;
                since_best = 0;
                HIP_CHECK(hipMemcpyAsync(best.p, comm.p, sizeof(i32) * n, hipMemcpyDeviceToDevice, st));
            } else if (++since_best >= 3)
                break;
            if (hs[3] == 0.0) break;    // nothing wants to move
            if (hs[0] == 0.0) continue; // everything that wants to is off turn: the next round is theirs
            hipLaunchKernelGGL(lv_apply_kernel, dim3(gv), dim3(256), 0, st, comm.p, newcomm.p, k.p, n, tot.p, size.p);
        }
    } else {
        // no edge between two vertices: the singletons stay.  in = sum_v self_v, tot_v = k_v
        best_q = 0.0;
        if (m2 > 0.0) {
            hipLaunchKernelGGL(lv_totsq_kernel, dim3(gv), dim3(256), 0, st, tot.p, size.p, n, stats.p);
            HIP_CHECK(hipMemcpyAsync(hs, stats.p, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            best_q = 1.0 - hs[2] / (m2 * m2); // len == 0: k_v = self_v, so "in" is m2 itself
        }
        HIP_CHECK(hipMemcpyAsync(best.p, comm.p, sizeof(i32) * n, hipMemcpyDeviceToDevice, st));
    }
    // renumber 0.. in ascending order of the surviving community ids
    used.ensure(n + 1); newid.ensure(n + 1); out.ensure(n);
    HIP_CHECK(hipMemsetAsync(used.p, 0, sizeof(i32) * (n + 1), st));
    hipLaunchKernelGGL(lv_used_kernel, dim3(gv), dim3(256), 0, st, best.p, n, used.p);
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, used.p, newid.p, (i32)0, (size_t)(n + 1), rocprim::plus<i32>(), st));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::exclusive_scan(c->sort_tmp.p, bytes, used.p, newid.p, (i32)0, (size_t)(n + 1), rocprim::plus<i32>(), st));
    }
    hipLaunchKernelGGL(lv_renumber_kernel, dim3(gv), dim3(256), 0, st, best.p, newid.p, n, out.p);
    i32 nc = 0;
    HIP_CHECK(hipMemcpyAsync(&nc, newid.p + n, sizeof(i32), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st)); // (the pass's buffers go with this frame)
    *n_comm = nc;
    *quality = best_q;
    *rounds_out = rounds;
}

// h = g contracted by comm (g.n entries in 0 .. nc-1, every id in use)
static void lv_contract(cge_ctx *c, const LvGraph &g, const i64 *comm, i64 nc, LvGraph &h) {
    hipStream_t st = c->stream;
    const i64 total = g.len + g.n;
    if (total >= INT32_MAX) CGE_THROW(CGE_E_ARG, "louvain: a level's adjacency is beyond 32-bit positions");
    int cb = 1;
    while (((i64)1 << cb) < nc) cb++;
    DevBuf<unsigned long long> keys, skeys;
    DevBuf<double> vals, svals;
    DevBuf<i32> flag, ridx, start;
    keys.ensure(total); skeys.ensure(total); vals.ensure(total); svals.ensure(total);
    flag.ensure(total + 1); ridx.ensure(total + 1);
    hipLaunchKernelGGL(lv_ckeys_kernel, dim3(grid_for(total, 256, 1 << 16)), dim3(256), 0, st, g.off.p, g.adj.p,
                       g.weighted ? g.aw.p : nullptr, g.self.p, comm, g.n, g.len, cb, keys.p, vals.p);
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, keys.p, skeys.p, vals.p, svals.p, (size_t)total, 0u, (unsigned)(2 * cb), st));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::radix_sort_pairs(c->sort_tmp.p, bytes, keys.p, skeys.p, vals.p, svals.p, (size_t)total, 0u, (unsigned)(2 * cb), st));
    }
    hipLaunchKernelGGL(lv_heads_kernel, dim3((unsigned)((total + 256) / 256)), dim3(256), 0, st, skeys.p, total, flag.p);
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, flag.p, ridx.p, (i32)0, (size_t)(total + 1), rocprim::plus<i32>(), st));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::exclusive_scan(c->sort_tmp.p, bytes, flag.p, ridx.p, (i32)0, (size_t)(total + 1), rocprim::plus<i32>(), st));
    }
    i32 R32 = 0;
    HIP_CHECK(hipMemcpyAsync(&R32, ridx.p + total, sizeof(i32), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const i64 R = R32; // nc (C, C) runs + the coarse adjacency entries
    if (R < nc) CGE_THROW(CGE_E_ASSERT, "louvain: contraction lost a community");
    start.ensure(R + 1);
    hipLaunchKernelGGL(lv_starts_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, skeys.p, ridx.p, total, start.p);
    h.n = nc;
    h.len = R - nc;
    h.weighted = true;
    h.off.ensure(nc + 1); h.adj.ensure(h.len); h.aw.ensure(h.len); h.self.ensure(nc);
    hipLaunchKernelGGL(lv_runsum_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, skeys.p, svals.p, start.p, R, nc, cb,
                       h.off.p, h.adj.p, h.aw.p, h.self.p);
    HIP_CHECK(hipStreamSynchronize(st)); // (the sort's buffers go with this frame)
}

// level 1 alone: comm_out_host[v] in 0 .. *n_comm-1
void k_louvain_level1(cge_ctx *c, i64 *comm_out_host, i64 *n_comm, double *quality, i64 *rounds_out) {
    LvGraph g;
    DevBuf<i64> out;
    i64 nc = 0, rounds = 0;
    double q = 0.0;
    lv_build_csr(c, g);
    lv_pass(c, g, 1, out, &nc, &q, &rounds);
    HIP_CHECK(hipMemcpyAsync(comm_out_host, out.p, sizeof(i64) * c->n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n_comm) *n_comm = nc;
    if (quality) *quality = q;
    if (rounds_out) *rounds_out = rounds;
}

// The hierarchy: level L + 1 is a pass on the contraction of level L.  It ends at the first level whose partition has as many
// communities as its graph has vertices (nothing merged; that level is not reported -- except level 1, which always is), or at
// max_levels > 0.  Every reported level after the first has strictly fewer communities than the one before, so no cap is needed.
// Row l of comm_out_host (levels_cap x n, may be NULL with levels_cap 0) = level l + 1's community of every ORIGINAL vertex.
// Returns the number of levels; rows and scalars are written for the first levels_cap of them
i64 k_louvain_levels(cge_ctx *c, i64 max_levels, i64 levels_cap, i64 *comm_out_host, i64 *n_comm, double *quality, i64 *rounds_out) {
    const i64 n = c->n;
    hipStream_t st = c->stream;
    LvGraph g, h;
    DevBuf<i64> comp, out;
    lv_build_csr(c, g);
    i64 n_levels = 0;
    for (int level = 1;; level++) {
        i64 nc = 0, rounds = 0;
        double q = 0.0;
        {
            const std::string name = "louvain_pass_L" + std::to_string(level);
            ScopedKernelTimer kt(c, name.c_str());
            lv_pass(c, g, level, out, &nc, &q, &rounds);
        }
        if (level > 1 && nc == g.n) break; // nothing merged
        if (level == 1) comp.swap(out);
        else hipLaunchKernelGGL(lv_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, comp.p, out.p, n);
        if (n_levels < levels_cap) {
            HIP_CHECK(hipMemcpyAsync(comm_out_host + n_levels * n, comp.p, sizeof(i64) * n, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            n_comm[n_levels] = nc;
            quality[n_levels] = q;
            rounds_out[n_levels] = rounds;
        }
        n_levels++;
        if ((max_levels > 0 && n_levels >= max_levels) || nc == g.n) break;
        {
            const std::string name = "louvain_contract_L" + std::to_string(level + 1);
            ScopedKernelTimer kt(c, name.c_str());
            lv_contract(c, g, level == 1 ? comp.p : out.p, nc, h);
        }
        g.off.swap(h.off); g.adj.swap(h.adj); g.aw.swap(h.aw); g.self.swap(h.self);
        g.n = h.n; g.len = h.len; g.weighted = true;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    return n_levels;
}
