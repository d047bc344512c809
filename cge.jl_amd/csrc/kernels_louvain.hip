// kernels_louvain.hip -- Louvain on the resident graph: level 1 is the communities `louvain_clust` writes to <file>.ecg
// when the command line has no `-c` (src/clustering.jl:14-68, src/auxilary.jl:115-121); the further
// levels (the reference's executable computes them all, `louvain -l -1`, and `hierarchy -l 1` throws them away,
// src/clustering.jl:20-24) are the same pass on the graph contracted by the level before (k_louvain_levels, below).
// ECG (k_ecg, at the end) is an ensemble of level-1 passes under relabelled vertices, in lock-step groups, and one hierarchy on the
// graph reweighted by their agreement.
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
// Members of a group (cge_ecg; everything else is a group of one): member g = blockIdx.y of the keys / decide / apply / tot^2
// kernels works on slice g of the per-member arrays (comm, newcomm, tot, size: n each; keys, sorted keys and weights: len each;
// stats: 5 each) and leaves them alone when bit g of `mask` is clear -- a member that has stopped keeps its state.  GROUP = false is
// the plain pass: none of this is compiled in, so cge_louvain and cge_louvain_levels run the instructions they ran before
template <bool GROUP>
__global__ void lv_keys_kernel(const i32 *__restrict__ adj, const i32 *__restrict__ comm, i64 len, unsigned *__restrict__ keys, i64 n,
                               unsigned long long mask) {
    if (GROUP) {
        const i64 g = blockIdx.y;
        if (!((mask >> g) & 1ull)) return;
        comm += g * n;
        keys += g * len;
    }
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < len; q += stride) keys[q] = (unsigned)comm[adj[q]];
}
// one thread per vertex: the runs of its community-sorted adjacency segment -> the community of largest gain.
// stats[0] += moves, stats[1] += sum_v (k_{v,own} + self_v)  (the "in" part of the modularity of the CURRENT partition),
// stats[3] += vertices that want to move: a strictly better community that the singleton guard allows, on turn or not
// SKIP (levels >= 2): a vertex whose segment is longer than `ell` is left to lv_decide_wave_kernel
// rank (members of cge_ecg; NULL: the identity): the vertex's name in the member's relabelled graph.  The member starts from
// comm[v] = rank[v], so the labels -- and with them the singleton guard and the smallest-id rule -- live in rank space already;
// the turn bit hashes the rank
template <bool SKIP, bool GROUP>
__global__ void lv_decide_kernel(const i32 *__restrict__ off, const unsigned *__restrict__ skeys, const double *__restrict__ saw,
                                 const double *__restrict__ self, const double *__restrict__ k, const double *__restrict__ tot,
                                 const i32 *__restrict__ size, const i32 *__restrict__ comm, i64 n, double m2, int round,
                                 i32 *__restrict__ newcomm, double *__restrict__ stats, i32 ell, const i32 *__restrict__ rank, i64 len,
                                 unsigned long long mask) {
    if (GROUP) {
        const i64 g = blockIdx.y;
        if (!((mask >> g) & 1ull)) return;
        skeys += g * len;
        if (saw) saw += g * len;
        tot += g * n; size += g * n; comm += g * n; newcomm += g * n;
        stats += g * 5;
        rank += g * n;
    }
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
        const unsigned name = GROUP ? (unsigned)rank[v] : (unsigned)v;
        const bool my_turn = (((name * 2654435761u) >> 15) & 1u) == (unsigned)(round & 1);
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
template <bool GROUP>
__global__ void lv_apply_kernel(i32 *__restrict__ comm, const i32 *__restrict__ newcomm, const double *__restrict__ k, i64 n,
                                double *__restrict__ tot, i32 *__restrict__ size, unsigned long long mask) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    if (GROUP) {
        const i64 g = blockIdx.y;
        if (!((mask >> g) & 1ull)) return;
        comm += g * n; newcomm += g * n; tot += g * n; size += g * n;
    }
    const i32 a = comm[v], b = newcomm[v];
    if (a == b) return;
    unsafeAtomicAdd(&tot[a], -k[v]);
    unsafeAtomicAdd(&tot[b], k[v]);
    atomicAdd(&size[a], -1);
    atomicAdd(&size[b], 1);
    comm[v] = b;
}
// stats[2] += sum_c tot_c^2 over the non-empty communities
template <bool GROUP>
__global__ void lv_totsq_kernel(const double *__restrict__ tot, const i32 *__restrict__ size, i64 n, double *__restrict__ stats,
                                unsigned long long mask) {
    if (GROUP) {
        const i64 g = blockIdx.y;
        if (!((mask >> g) & 1ull)) return;
        tot += g * n; size += g * n;
        stats += g * 5;
    }
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
// a member's start: the singletons under its names.  rank is a permutation, so every slot of tot / size is written
__global__ void lv_member_init_kernel(const i32 *__restrict__ rank, const double *__restrict__ k, i64 n, i32 *__restrict__ comm,
                                      double *__restrict__ tot, i32 *__restrict__ size) {
    const i64 g = blockIdx.y, v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const i32 r = rank[g * n + v];
    comm[g * n + v] = r;
    tot[g * n + r] = k[v];
    size[g * n + r] = 1;
}
// segment v of member g starts at g * len + off[v]; entry G * n closes the last one
__global__ void lv_group_offsets_kernel(const i32 *__restrict__ off, i64 n, i64 len, i64 G, i32 *__restrict__ goff) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i <= G * n; i += stride) goff[i] = (i32)((i / n) * len + off[i % n]);
}

// ---- ECG (Poulin & Theberge): K relabelled level-1 members, the 2-core, edges reweighted by co-membership -----------------------
// splitmix64
__host__ __device__ static inline unsigned long long ecg_mix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// a member's names: the position of v among the vertices ordered by (mix(base ^ v), v) -- the keys with the values 0 .. n-1 through
// one stable radix sort, then the sorted positions scattered back
__global__ void ecg_keys_kernel(unsigned long long base, i64 n, unsigned long long *__restrict__ keys, i32 *__restrict__ vals) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    keys[v] = ecg_mix(base ^ (unsigned long long)v);
    vals[v] = (i32)v;
}
__global__ void ecg_rank_kernel(const i32 *__restrict__ sorted, i64 n, i32 *__restrict__ rank) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rank[sorted[i]] = (i32)i;
}
// the members' labels are kept member-minor, labels[v * K + r]: at K = 16 a vertex's labels are one 64-byte line, and the
// co-membership count of an adjacency entry is two line reads
__global__ void ecg_labels_kernel(const i32 *__restrict__ best, i64 n, i64 K, i64 r0, i64 G, i32 *__restrict__ labels) {
    const i64 g = blockIdx.y, v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) labels[v * K + r0 + g] = best[g * n + v];
}
__global__ void ecg_member_kernel(const i32 *__restrict__ labels, i64 n, i64 K, i64 r, i32 *__restrict__ out) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) out[v] = labels[v * K + r];
}
// the 2-core on adjacency entries (repeated edges are separate entries, self loops are none): rounds of mark -- every live vertex
// with fewer than 2 live entries, as the degrees stood when the round began -- and apply, which takes the marked out of their
// neighbours' degrees.  flag (one word per round) is set by a round that marks anything
__global__ void ecg_peel_init_kernel(const i32 *__restrict__ off, i64 n, i32 *__restrict__ deg, i32 *__restrict__ alive) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) { deg[v] = off[v + 1] - off[v]; alive[v] = 1; }
}
__global__ void ecg_peel_mark_kernel(const i32 *__restrict__ deg, i32 *__restrict__ alive, i64 n, i32 *__restrict__ mark,
                                     i32 *__restrict__ flag) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const i32 go = alive[v] && deg[v] < 2;
    mark[v] = go;
    if (go) { alive[v] = 0; *flag = 1; }
}
__global__ void ecg_peel_apply_kernel(const i32 *__restrict__ off, const i32 *__restrict__ adj, const i32 *__restrict__ mark, i64 n,
                                      i32 *__restrict__ deg) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n || !mark[v]) return;
    for (i32 q = off[v]; q < off[v + 1]; q++) atomicSub(&deg[adj[q]], 1);
}
// w_min + (1 - w_min) c / K with c the members that have u and v in one community, both in the 2-core; w_min otherwise
__device__ __forceinline__ double ecg_weight(i64 u, i64 v, const i32 *__restrict__ labels, const i32 *__restrict__ alive, i64 K,
                                             double w_min) {
    if (!(alive[u] && alive[v])) return w_min;
    int cnt = 0;
    for (i64 r = 0; r < K; r++) cnt += labels[u * K + r] == labels[v * K + r] ? 1 : 0;
    return w_min + (1.0 - w_min) * (double)cnt / (double)K;
}
// per adjacency entry, straight from (v, adj[q]) (v by bisection of off)
__global__ void ecg_entry_weights_kernel(const i32 *__restrict__ off, const i32 *__restrict__ adj, const i32 *__restrict__ labels,
                                         const i32 *__restrict__ alive, i64 n, i64 len, i64 K, double w_min, double *__restrict__ aw) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < len; j += stride) {
        i64 lo = 0, hi = n; // off[lo] <= j, and hi == n or off[hi] > j
        while (hi - lo > 1) {
            const i64 mid = (lo + hi) >> 1;
            if (off[mid] <= j) lo = mid; else hi = mid;
        }
        aw[j] = ecg_weight(lo, adj[j], labels, alive, K, w_min);
    }
}
// per original edge, in edge order (ew may be NULL); the self loops of a vertex all have one weight, so their sum in self[v] does
// not depend on the order of the additions
__global__ void ecg_edge_weights_kernel(const i32 *__restrict__ src, const i32 *__restrict__ dst, i64 m, const i32 *__restrict__ labels,
                                        const i32 *__restrict__ alive, i64 K, double w_min, double *__restrict__ ew,
                                        double *__restrict__ self) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const i32 u = src[e], v = dst[e];
        const double w = ecg_weight(u, v, labels, alive, K, w_min);
        if (ew) ew[e] = w;
        if (u == v) unsafeAtomicAdd(&self[u], w);
    }
}
// k_C of a contracted graph: its row sum plus its self loop, in ascending position
__global__ void lv_rowsum_kernel(const i32 *__restrict__ off, const double *__restrict__ aw, const double *__restrict__ self, i64 n,
                                 double *__restrict__ k) {
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double s = 0.0;
    for (i32 q = off[v]; q < off[v + 1]; q++) s += aw[q];
    k[v] = s + self[v];
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
#define ECG_AUTO_GROUP 16 // cge_ecg, option ecg_group = 0: at most this many members in lock-step

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

// One pass of local moving on g, or G of them in lock-step.  Level 1 decides every vertex in a lane; from level 2 on the
// segments longer than `ell` go to lv_decide_wave_kernel (the plain pass only).
// The group form (cge_ecg's members): G passes on the one graph in lock-step, member g under the vertex names rank[g * n + v]
// (NULL with G = 1: the plain pass).  Every round is one set of launches -- the member a grid dimension, the adjacency keys of
// all members in one segmented sort of G * n segments -- and one read-back of the G x 5 statistics; each member keeps its own best
// modularity, rounds without an improvement and best partition, and drops out of the launches' mask when it stops.
// best: G x n labels as the pass holds them (not renumbered); q, rounds: per member
static void lv_pass_group(cge_ctx *c, const LvGraph &g, int level, int G, const i32 *rank, DevBuf<i32> &best, double *q_out,
                          i64 *rounds_out) {
    const i64 n = g.n, len = g.len;
    const bool weighted = g.weighted;
    hipStream_t st = c->stream;
    const unsigned gv = (unsigned)((n + 255) / 256);
    const unsigned long long all = G >= 64 ? ~0ull : (1ull << G) - 1ull;
    const bool group = rank != nullptr; // the members' form of the kernels (a group of one member included)
    DevBuf<i32> comm, newcomm, size, longs, nlong_d, goff;
    DevBuf<unsigned> keys, skeys;
    DevBuf<double> saw, awg, k, tot, stats;
    const double *aw = weighted ? g.aw.p : nullptr;
    keys.ensure(G * len); skeys.ensure(G * len);
    if (weighted) saw.ensure(G * len);
    k.ensure(n); tot.ensure(G * n); comm.ensure(G * n); newcomm.ensure(G * n); size.ensure(G * n); best.ensure(G * n);
    stats.ensure(G * 5); // per member: moves, in, sum tot^2, wants, (m2 at the start; cleared every round)
    HIP_CHECK(hipMemsetAsync(stats.p, 0, sizeof(double) * 5, st));
    hipLaunchKernelGGL(lv_degree_kernel, dim3(gv), dim3(256), 0, st, g.off.p, aw, g.self.p, n, k.p, tot.p, comm.p, size.p, stats.p + 4);
    std::vector<double> hs((size_t)G * 5);
    HIP_CHECK(hipMemcpyAsync(hs.data(), stats.p, sizeof(double) * 5, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const double m2 = hs[4];
    int bits = 1;
    while (((i64)1 << bits) < n) bits++;
    if (rank) hipLaunchKernelGGL(lv_member_init_kernel, dim3(gv, G), dim3(256), 0, st, rank, k.p, n, comm.p, tot.p, size.p);
    // the segments of all members, and the weights once per member (the sort's values), when there is more than one
    const i32 *seg = g.off.p;
    const double *awin = aw;
    if (G > 1) {
        goff.ensure(G * n + 1);
        hipLaunchKernelGGL(lv_group_offsets_kernel, dim3(grid_for(G * n + 1, 256)), dim3(256), 0, st, g.off.p, n, len, (i64)G, goff.p);
        seg = goff.p;
        if (weighted) {
            awg.ensure(G * len);
            for (int m = 0; m < G; m++)
                HIP_CHECK(hipMemcpyAsync(awg.p + m * len, aw, sizeof(double) * len, hipMemcpyDeviceToDevice, st));
            awin = awg.p;
        }
    }
    const unsigned nseg = (unsigned)(G * n), nkeys = (unsigned)(G * len);
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
    std::vector<double> best_q((size_t)G, -1e300);
    std::vector<int> since_best((size_t)G, 0);
    for (int m = 0; m < G; m++) rounds_out[m] = 0;
    if (m2 > 0.0 && len > 0) {
        unsigned long long active = all;
        for (int round = 0; round < 200 && active; round++) {
            hipLaunchKernelGGL(group ? lv_keys_kernel<true> : lv_keys_kernel<false>, dim3(grid_for(len, 256), G), dim3(256), 0, st, g.adj.p,
                               comm.p, len, keys.p, n, active);
            size_t bytes = 0;
            if (weighted) {
                HIP_CHECK(rocprim::segmented_radix_sort_pairs(nullptr, bytes, keys.p, skeys.p, awin, saw.p, nkeys, nseg, seg, seg + 1, 0,
                                                              bits, st));
                c->sort_tmp.ensure(bytes);
                HIP_CHECK(rocprim::segmented_radix_sort_pairs(c->sort_tmp.p, bytes, keys.p, skeys.p, awin, saw.p, nkeys, nseg, seg,
                                                              seg + 1, 0, bits, st));
            } else {
                HIP_CHECK(rocprim::segmented_radix_sort_keys(nullptr, bytes, keys.p, skeys.p, nkeys, nseg, seg, seg + 1, 0, bits, st));
                c->sort_tmp.ensure(bytes);
                HIP_CHECK(rocprim::segmented_radix_sort_keys(c->sort_tmp.p, bytes, keys.p, skeys.p, nkeys, nseg, seg, seg + 1, 0, bits, st));
            }
            HIP_CHECK(hipMemsetAsync(stats.p, 0, sizeof(double) * 5 * G, st));
            if (nlong > 0) {
                hipLaunchKernelGGL((lv_decide_kernel<true, false>), dim3(gv), dim3(256), 0, st, g.off.p, skeys.p, saw.p, g.self.p, k.p, tot.p,
                                   size.p, comm.p, n, m2, round, newcomm.p, stats.p, ell, (const i32 *)nullptr, len, 1ull);
                hipLaunchKernelGGL(lv_decide_wave_kernel, dim3(grid_for(nlong, 4)), dim3(256), 0, st, longs.p, nlong, g.off.p, skeys.p,
                                   saw.p, g.self.p, k.p, tot.p, size.p, comm.p, m2, round, newcomm.p, stats.p);
            } else
                hipLaunchKernelGGL((group ? lv_decide_kernel<false, true> : lv_decide_kernel<false, false>), dim3(gv, G), dim3(256), 0, st,
                                   g.off.p, skeys.p, weighted ? saw.p : nullptr,
                                   g.self.p, k.p, tot.p, size.p, comm.p, n, m2, round, newcomm.p, stats.p, 0, rank, len, active);
            hipLaunchKernelGGL(group ? lv_totsq_kernel<true> : lv_totsq_kernel<false>, dim3(gv, G), dim3(256), 0, st, tot.p, size.p, n,
                               stats.p, active);
            HIP_CHECK(hipMemcpyAsync(hs.data(), stats.p, sizeof(double) * 5 * G, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            unsigned long long apply = 0;
            for (int m = 0; m < G; m++) {
                const unsigned long long bit = 1ull << m;
                if (!(active & bit)) continue;
                const double *h = hs.data() + 5 * m;
                rounds_out[m] = round + 1;
                const double q = h[1] / m2 - h[2] / (m2 * m2); // modularity of the partition this round STARTED from
                if (q > best_q[m] + 1e-6) {
                    best_q[m] = q;
                    since_best[m] = 0;
                    HIP_CHECK(hipMemcpyAsync(best.p + m * n, comm.p + m * n, sizeof(i32) * n, hipMemcpyDeviceToDevice, st));
                } else if (++since_best[m] >= 3) {
                    active &= ~bit;
                    continue;
                }
                if (h[3] == 0.0) active &= ~bit; // nothing wants to move
                else if (h[0] != 0.0) apply |= bit; // (else everything that wants to is off turn: the next round is theirs)
            }
            if (apply)
                hipLaunchKernelGGL(group ? lv_apply_kernel<true> : lv_apply_kernel<false>, dim3(gv, G), dim3(256), 0, st, comm.p,
                                   newcomm.p, k.p, n, tot.p, size.p, apply);
        }
    } else {
        // no edge between two vertices: the singletons stay.  in = sum_v self_v, tot_v = k_v (under any names)
        double q = 0.0;
        if (m2 > 0.0) {
            hipLaunchKernelGGL(lv_totsq_kernel<false>, dim3(gv), dim3(256), 0, st, tot.p, size.p, n, stats.p, 1ull);
            HIP_CHECK(hipMemcpyAsync(hs.data(), stats.p, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            q = 1.0 - hs[2] / (m2 * m2); // len == 0: k_v = self_v, so "in" is m2 itself
        }
        for (int m = 0; m < G; m++) best_q[m] = q;
        HIP_CHECK(hipMemcpyAsync(best.p, comm.p, sizeof(i32) * n * G, hipMemcpyDeviceToDevice, st));
    }
    for (int m = 0; m < G; m++) q_out[m] = best_q[m];
    HIP_CHECK(hipStreamSynchronize(st)); // (the pass's buffers go with this frame)
}

// labels (n, any ids in 0 .. n-1) -> out[v] in 0 .. *n_comm-1, in ascending order of the ids in use
static void lv_renumber(cge_ctx *c, const i32 *labels, i64 n, DevBuf<i64> &out, i64 *n_comm) {
    hipStream_t st = c->stream;
    const unsigned gv = (unsigned)((n + 255) / 256);
    DevBuf<i32> used, newid;
    used.ensure(n + 1); newid.ensure(n + 1); out.ensure(n);
    HIP_CHECK(hipMemsetAsync(used.p, 0, sizeof(i32) * (n + 1), st));
    hipLaunchKernelGGL(lv_used_kernel, dim3(gv), dim3(256), 0, st, labels, n, used.p);
    {
        size_t bytes = 0;
        HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, used.p, newid.p, (i32)0, (size_t)(n + 1), rocprim::plus<i32>(), st));
        c->sort_tmp.ensure(bytes);
        HIP_CHECK(rocprim::exclusive_scan(c->sort_tmp.p, bytes, used.p, newid.p, (i32)0, (size_t)(n + 1), rocprim::plus<i32>(), st));
    }
    hipLaunchKernelGGL(lv_renumber_kernel, dim3(gv), dim3(256), 0, st, labels, newid.p, n, out.p);
    i32 nc = 0;
    HIP_CHECK(hipMemcpyAsync(&nc, newid.p + n, sizeof(i32), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st)); // (the buffers go with this frame)
    *n_comm = nc;
}

// the plain pass, a group of one under the vertices' own names: out[v] in 0 .. *n_comm-1 on the device (ascending order of the old
// community ids, as the reference's renumbering), *quality = modularity of the returned partition, *rounds_out = synchronous rounds
static void lv_pass(cge_ctx *c, const LvGraph &g, int level, DevBuf<i64> &out, i64 *n_comm, double *quality, i64 *rounds_out) {
    DevBuf<i32> best;
    lv_pass_group(c, g, level, 1, nullptr, best, quality, rounds_out);
    lv_renumber(c, best.p, g.n, out, n_comm);
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
// g is level 1's graph and is used up.  `last` (may be NULL): the last reported level stays on the device in last->comm, with its
// community count and modularity
struct LvLast {
    DevBuf<i64> comm;
    i64 n_comm = 0;
    double q = 0.0;
};
static i64 lv_hierarchy(cge_ctx *c, LvGraph &g, const char *timer, i64 max_levels, i64 levels_cap, i64 *comm_out_host, i64 *n_comm,
                        double *quality, i64 *rounds_out, LvLast *last) {
    const i64 n = g.n;
    hipStream_t st = c->stream;
    LvGraph h;
    DevBuf<i64> comp, out;
    i64 n_levels = 0;
    for (int level = 1;; level++) {
        i64 nc = 0, rounds = 0;
        double q = 0.0;
        {
            const std::string name = std::string(timer) + "_pass_L" + std::to_string(level);
            ScopedKernelTimer kt(c, name.c_str());
            lv_pass(c, g, level, out, &nc, &q, &rounds);
        }
        if (level > 1 && nc == g.n) break; // nothing merged
        if (level == 1) comp.swap(out);
        else hipLaunchKernelGGL(lv_compose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, comp.p, out.p, n);
        if (last) { last->n_comm = nc; last->q = q; }
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
            const std::string name = std::string(timer) + "_contract_L" + std::to_string(level + 1);
            ScopedKernelTimer kt(c, name.c_str());
            lv_contract(c, g, level == 1 ? comp.p : out.p, nc, h);
        }
        g.off.swap(h.off); g.adj.swap(h.adj); g.aw.swap(h.aw); g.self.swap(h.self);
        g.n = h.n; g.len = h.len; g.weighted = true;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    if (last) last->comm.swap(comp);
    return n_levels;
}
i64 k_louvain_levels(cge_ctx *c, i64 max_levels, i64 levels_cap, i64 *comm_out_host, i64 *n_comm, double *quality, i64 *rounds_out) {
    LvGraph g;
    lv_build_csr(c, g);
    return lv_hierarchy(c, g, "louvain", max_levels, levels_cap, comm_out_host, n_comm, quality, rounds_out, nullptr);
}

// ---- ECG on the resident graph ------------------------------------------------------------------------------------------------------
// Departures from the published algorithm: the members are this file's synchronous level-1 passes, diversified by relabelling
// alone (the names decide ties, the singleton guard and the turn of a vertex), on the graph's own weights; the 2-core counts
// adjacency entries, so a repeated edge keeps both its ends.
//
// modularity of `comm` (n, 0 .. nc-1, every id in use) on g: g contracted by it has in_C in self[C] and tot_C as its row sum -- sums
// in ascending sorted position -- and the nc terms are added on the host in ascending C
static double lv_modularity(cge_ctx *c, const LvGraph &g, const i64 *comm, i64 nc) {
    hipStream_t st = c->stream;
    LvGraph h;
    DevBuf<double> k;
    lv_contract(c, g, comm, nc, h);
    k.ensure(nc);
    hipLaunchKernelGGL(lv_rowsum_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, h.off.p, h.aw.p, h.self.p, nc, k.p);
    std::vector<double> in((size_t)nc), tot((size_t)nc);
    HIP_CHECK(hipMemcpyAsync(in.data(), h.self.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(tot.data(), k.p, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    double in_sum = 0.0, m2 = 0.0, sq = 0.0;
    for (i64 C = 0; C < nc; C++) { in_sum += in[C]; m2 += tot[C]; sq += tot[C] * tot[C]; }
    return m2 > 0.0 ? in_sum / m2 - sq / (m2 * m2) : 0.0;
}

// members of a group: what the free memory holds (half of it, the sorts' scratch aside), G * len < 2^31, the option's cap
static int ecg_group_size(cge_ctx *c, const LvGraph &g, i64 K) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const double per = (double)g.len * (g.weighted ? 32.0 : 12.0) + (double)g.n * 32.0 + 64.0; // keys, sorted, weights twice, scratch; labels
    i64 G = (i64)std::min((double)K, std::max(1.0, 0.5 * (double)free_b / per));
    G = std::min(G, (i64)((INT32_MAX - 1) / std::max<i64>(std::max(g.len, g.n), 1)));
    if (c->opt_ecg_group > 0) G = std::min<i64>(G, c->opt_ecg_group);
    else G = std::min<i64>(G, ECG_AUTO_GROUP);
    return (int)std::max<i64>(G, 1);
}

void k_ecg(cge_ctx *c, i64 K, double w_min, i64 seed, i64 final_level, bool members_only, const EcgHostOut &o) {
    const i64 n = c->n, m = c->m;
    hipStream_t st = c->stream;
    const unsigned gv = (unsigned)((n + 255) / 256);
    LvGraph g;
    lv_build_csr(c, g);
    const i64 len = g.len;
    // ranks: K x n
    DevBuf<i32> rank, labels, alive;
    rank.ensure(K * n); labels.ensure(K * n); alive.ensure(n);
    {
        ScopedKernelTimer kt(c, "ecg_ranks");
        DevBuf<unsigned long long> keys, skeys;
        DevBuf<i32> vals, svals;
        keys.ensure(n); skeys.ensure(n); vals.ensure(n); svals.ensure(n);
        for (i64 r = 0; r < K; r++) {
            const unsigned long long base = ecg_mix((unsigned long long)seed ^ ecg_mix((unsigned long long)r));
            hipLaunchKernelGGL(ecg_keys_kernel, dim3(gv), dim3(256), 0, st, base, n, keys.p, vals.p);
            size_t bytes = 0;
            HIP_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, keys.p, skeys.p, vals.p, svals.p, (size_t)n, 0u, 64u, st));
            c->sort_tmp.ensure(bytes);
            HIP_CHECK(rocprim::radix_sort_pairs(c->sort_tmp.p, bytes, keys.p, skeys.p, vals.p, svals.p, (size_t)n, 0u, 64u, st));
            hipLaunchKernelGGL(ecg_rank_kernel, dim3(gv), dim3(256), 0, st, svals.p, n, rank.p + r * n);
        }
        HIP_CHECK(hipStreamSynchronize(st)); // (the sort's buffers go with this frame)
    }
    // members, in lock-step groups
    std::vector<double> mq((size_t)K);
    std::vector<i64> mrounds((size_t)K);
    c->stat_ecg_groups = 0;
    {
        ScopedKernelTimer kt(c, "ecg_members");
        const int G = ecg_group_size(c, g, K);
        DevBuf<i32> best;
        for (i64 r0 = 0; r0 < K; r0 += G) {
            const int Gr = (int)std::min<i64>(G, K - r0);
            lv_pass_group(c, g, 1, Gr, rank.p + r0 * n, best, mq.data() + r0, mrounds.data() + r0);
            hipLaunchKernelGGL(ecg_labels_kernel, dim3(gv, Gr), dim3(256), 0, st, best.p, n, K, r0, (i64)Gr, labels.p);
            c->stat_ecg_groups++;
        }
        HIP_CHECK(hipStreamSynchronize(st));
    }
    c->stat_ecg_member_rounds = 0;
    for (i64 r = 0; r < K; r++) c->stat_ecg_member_rounds += mrounds[r];
    // the 2-core: several rounds per read of the flags, so that a long path does not cost one synchronisation per round
    {
        ScopedKernelTimer kt(c, "ecg_peel");
        const int R = 16;
        DevBuf<i32> deg, mark, flags;
        deg.ensure(n); mark.ensure(n); flags.ensure(R);
        hipLaunchKernelGGL(ecg_peel_init_kernel, dim3(gv), dim3(256), 0, st, g.off.p, n, deg.p, alive.p);
        i64 peel_rounds = 0;
        for (bool more = true; more;) {
            i32 hf[R];
            HIP_CHECK(hipMemsetAsync(flags.p, 0, sizeof(i32) * R, st));
            for (int r = 0; r < R; r++) {
                hipLaunchKernelGGL(ecg_peel_mark_kernel, dim3(gv), dim3(256), 0, st, deg.p, alive.p, n, mark.p, flags.p + r);
                hipLaunchKernelGGL(ecg_peel_apply_kernel, dim3(gv), dim3(256), 0, st, g.off.p, g.adj.p, mark.p, n, deg.p);
            }
            HIP_CHECK(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            for (int r = 0; r < R; r++) peel_rounds += hf[r]; // (a round that removes nothing is the last that could)
            more = hf[R - 1] != 0;
        }
        c->stat_ecg_peel_rounds = peel_rounds;
    }
    if (o.member_comm) { // the testing hook: every member renumbered as a pass is
        DevBuf<i32> one;
        DevBuf<i64> out;
        one.ensure(n);
        for (i64 r = 0; r < K; r++) {
            hipLaunchKernelGGL(ecg_member_kernel, dim3(gv), dim3(256), 0, st, labels.p, n, K, r, one.p);
            lv_renumber(c, one.p, n, out, o.member_nc + r);
            HIP_CHECK(hipMemcpyAsync(o.member_comm + r * n, out.p, sizeof(i64) * n, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            o.member_q[r] = mq[r];
            o.member_rounds[r] = mrounds[r];
        }
    }
    if (o.core) {
        HIP_CHECK(hipMemcpyAsync(o.core, alive.p, sizeof(i32) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (members_only) return;
    // the reweighted graph: level 1's offsets and adjacency, the ECG weight per entry, the self loops' per vertex
    LvGraph f;
    {
        ScopedKernelTimer kt(c, "ecg_weights");
        DevBuf<double> ew;
        f.n = n; f.len = len; f.weighted = true;
        f.off.ensure(n + 1); f.adj.ensure(len); f.aw.ensure(len); f.self.ensure(n);
        HIP_CHECK(hipMemcpyAsync(f.off.p, g.off.p, sizeof(i32) * (n + 1), hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemcpyAsync(f.adj.p, g.adj.p, sizeof(i32) * len, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemsetAsync(f.self.p, 0, sizeof(double) * n, st));
        if (len > 0)
            hipLaunchKernelGGL(ecg_entry_weights_kernel, dim3(grid_for(len, 256, 1 << 16)), dim3(256), 0, st, g.off.p, g.adj.p, labels.p,
                               alive.p, n, len, K, w_min, f.aw.p);
        if (o.edge_w) ew.ensure(m);
        hipLaunchKernelGGL(ecg_edge_weights_kernel, dim3(grid_for(m, 256, 1 << 16)), dim3(256), 0, st, c->src.p, c->dst.p, m, labels.p,
                           alive.p, K, w_min, o.edge_w ? ew.p : nullptr, f.self.p);
        if (o.edge_w) HIP_CHECK(hipMemcpyAsync(o.edge_w, ew.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    LvLast last;
    {
        ScopedKernelTimer kt(c, "ecg_hierarchy");
        c->stat_ecg_levels = lv_hierarchy(c, f, "ecg", std::max<i64>(final_level, 0), 0, nullptr, nullptr, nullptr, nullptr, &last);
    }
    HIP_CHECK(hipMemcpyAsync(o.comm, last.comm.p, sizeof(i64) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    {
        ScopedKernelTimer kt(c, "ecg_modularity");
        *o.q = lv_modularity(c, g, last.comm.p, last.n_comm);
    }
    *o.n_comm = last.n_comm;
    if (o.q_ecg) *o.q_ecg = last.q;
}
