// diameter_host.cpp -- the exact point-set diameter `hi = maximum(full_graph_D)` (src/divergence.jl:104-113): the largest dist()
// value of any two rows of the resident embedding, with the reference's bits whatever the data.  DESIGN.md 4.5 has the method
// and its proofs; this file holds, top to bottom:
//   gram_delta, dm_eval_pairs, dm_collect   the near-ties of an arg-max launch, evaluated in dist()'s own arithmetic;
//   host_diameter_brute                     every pair tile of the embedding (this rank's share), no pruning;
//   dm_prepare, dm_bound_pass               the landmark-sorted layout and the bounds P[a][r] >= max_{i in a} ||x_i - ref_r||^2;
//   host_diameter_pruned                    branch and bound over landmark pairs, a list of stages sharing a DmSearch;
//   host_diameter_landmarks                 the entry of a score: pruned, brute force where the bounds prune too little;
//   host_diameter_bounds_test               the testing hook of the bound passes;
//   host_ref_dist2_test                     the testing hook of the reference points' distance matrix.
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>

#include "common.hpp"

namespace {
// the answer: the largest dist() value of the pairs evaluated so far; ties go to the smallest (i, j)
struct ExactBest {
    double hi = -1.0;
    i64 i = 0, j = 0;
    void offer(double v, i64 a, i64 b) {
        if (a > b) std::swap(a, b);
        if (v > hi || (v == hi && (a < i || (a == i && b < j)))) { hi = v; i = a; j = b; }
    }
};
// while one lives, the launch wrappers (they enqueue on c->stream) work on the side stream
struct SideStream {
    cge_ctx *c;
    explicit SideStream(cge_ctx *c_) : c(c_) { std::swap(c->stream, c->copy_stream); }
    ~SideStream() { std::swap(c->stream, c->copy_stream); }
};
} // namespace

// THE ARG-MAX IS RANKED IN ONE ARITHMETIC AND `hi` IS DEFINED IN ANOTHER.  The tile kernels rank pairs by the Gram value
// g(p) = fl(fl(r_i + r_j) - 2 <x_i, x_j>) of the centred rows; the reference takes the maximum of s(p), dist()'s sequential sum of
// the squared differences of the rows as given.  Against the exact squared distance D(p), with u = 2^-53, K = dpad >= d and
// r = the largest squared norm of a centred row:
//   centring rounds every coordinate once: D moves by at most 2 sqrt(D) u (|x_i| + |x_j|) <= 4 u (r_i + r_j);
//   the norms are sums of K squares: (K + 1) u (r_i + r_j);  the K-term product sum, in whatever order the matrix instruction
//   adds it: 2 K u |x_i||x_j| <= K u (r_i + r_j);  the two final operations: <= 4 u (r_i + r_j)
//       => |g(p) - D(p)| <= (2K + 9) u (r_i + r_j);
//   s(p) is a sum of d non-negative terms, each a rounded difference squared: |s(p) - D(p)| <= (d + 2) u D(p) <= 2 (d + 2) u (r_i + r_j)
//       => |g(p) - s(p)| <= (4K + 13) u (r_i + r_j) <= (4K + 13) 2^-52 r =: eta   (any other summation order of s obeys it too).
// If p* maximises s and q maximises g, g(p*) >= s(p*) - eta >= s(q) - eta >= g(q) - 2 eta.  So every pair that can hold the
// reference's maximum has a Gram value of at least  g(q) - delta,  delta = (8K + 32) 2^-52 r  (the +6 covers the second-order
// terms: K u < 2^-43).  Those pairs -- one, unless the data is tied to the last bits -- are evaluated with dist()'s own arithmetic
// (k_pair_dist) and the largest VALUE wins, ties going to the smallest (i, j): the bits of the reference's `hi` whatever the
// data.  Evaluating more pairs than these cannot change the answer (each value is a genuine distance), so a lower threshold
// in an earlier round is harmless.
static double gram_delta(i64 dpad, double rmax) { return (double)(8 * dpad + 32) * 2.220446049250313e-16 * rmax; }

// dist() of `cnt` vertex pairs (global ids) into `eb`.  Option shard_rows: collective -- the ranks pool their pairs (a slot per
// rank in a zero-filled buffer, the words added: exact), fetch the rows from their owners the same way, and every rank
// evaluates every pair: all of them end with the same answer.
static void dm_eval_pairs(cge_ctx *c, const int2 *pairs, i64 cnt, ExactBest &eb) {
    const i64 d = c->d;
    hipStream_t st = c->stream;
    const i64 CH = 1 << 16;
    if (!c->rows_sharded) {
        std::vector<i32> ij;
        std::vector<double> val;
        for (i64 k0 = 0; k0 < cnt; k0 += CH) {
            const i64 kc = std::min(CH, cnt - k0);
            ij.resize(2 * kc);
            val.resize(kc);
            for (i64 k = 0; k < kc; k++) { ij[k] = pairs[k0 + k].x; ij[kc + k] = pairs[k0 + k].y; }
            c->nt_idx.ensure(2 * kc);
            c->nt_out.ensure(kc);
            HIP_CHECK(hipMemcpyAsync(c->nt_idx.p, ij.data(), sizeof(i32) * 2 * kc, hipMemcpyHostToDevice, st));
            k_pair_dist(c, c->Xr.p, d, c->nt_idx.p, c->nt_idx.p + kc, kc, 1.0, c->nt_out.p);
            HIP_CHECK(hipMemcpyAsync(val.data(), c->nt_out.p, sizeof(double) * kc, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st)); // (also: ij is reused)
            for (i64 k = 0; k < kc; k++) eb.offer(val[k], ij[k], ij[kc + k]);
        }
        return;
    }
    const int W = c->coll.world, me = c->coll.rank;
    const i64 RCH = 4096; // pairs per rank and step
    const i64 steps = (i64)cge_allreduce_scalar_max(c, (double)((cnt + RCH - 1) / RCH));
    std::vector<int2> all((size_t)W * RCH);
    std::vector<i32> loc, two;
    std::vector<double> val;
    for (i64 s = 0; s < steps; s++) {
        const i64 k0 = s * RCH, kc = std::max<i64>(0, std::min(RCH, cnt - k0));
        c->nt_pairs.ensure((size_t)W * RCH);
        HIP_CHECK(hipMemsetAsync(c->nt_pairs.p, 0, sizeof(int2) * W * RCH, st));
        std::vector<int2> mine(kc);
        for (i64 k = 0; k < kc; k++) mine[k] = make_int2(pairs[k0 + k].x + 1, pairs[k0 + k].y + 1); // (0 = no pair)
        if (kc > 0) HIP_CHECK(hipMemcpyAsync(c->nt_pairs.p + (size_t)me * RCH, mine.data(), sizeof(int2) * kc, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st)); // (`mine` leaves scope)
        cge_allreduce_dev(c, reinterpret_cast<double *>(c->nt_pairs.p), W * RCH, 2); // (an int2 is one 8-byte word)
        HIP_CHECK(hipMemcpyAsync(all.data(), c->nt_pairs.p, sizeof(int2) * W * RCH, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        loc.clear();
        std::vector<int2> got;
        for (const int2 &q : all)
            if (q.x > 0 && q.y > 0) {
                got.push_back(make_int2(q.x - 1, q.y - 1));
                loc.push_back(c->h_glob2loc[q.x - 1]);
                loc.push_back(c->h_glob2loc[q.y - 1]);
            }
        const i64 T = (i64)got.size();
        if (T == 0) continue; // (the same on every rank)
        two.resize(2 * T);
        for (i64 k = 0; k < T; k++) { two[k] = (i32)(2 * k); two[T + k] = (i32)(2 * k + 1); }
        val.resize(T);
        c->nt_idx.ensure(4 * T);
        c->nt_rows.ensure((size_t)2 * T * d);
        c->nt_out.ensure(T);
        HIP_CHECK(hipMemcpyAsync(c->nt_idx.p, loc.data(), sizeof(i32) * 2 * T, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(c->nt_idx.p + 2 * T, two.data(), sizeof(i32) * 2 * T, hipMemcpyHostToDevice, st));
        k_gather_rows_f64(c, c->Xr.p, c->n_loc, d, 1, c->nt_idx.p, 2 * T, c->nt_rows.p); // (rows of other ranks: zeros)
        cge_allreduce_dev(c, c->nt_rows.p, 2 * T * d, 2);
        k_pair_dist(c, c->nt_rows.p, d, c->nt_idx.p + 2 * T, c->nt_idx.p + 3 * T, T, 1.0, c->nt_out.p);
        HIP_CHECK(hipMemcpyAsync(val.data(), c->nt_out.p, sizeof(double) * T, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        // (pair_dist_kernel answers 0 for equal INDICES: here the two rows of a pair always differ in index, and equal rows give 0 anyway)
        for (i64 k = 0; k < T; k++) eb.offer(got[k].x == got[k].y ? 0.0 : val[k], got[k].x, got[k].y);
    }
}

// Every pair of the listed tiles whose Gram value reaches `thr`, handed to `flush` in lists of at most NT_CAP pairs.  `tl` = the
// tiles of the arg-max launch that can hold such a pair: those of the workgroups whose own best value reaches `thr` (wg[b]:
// workgroup b took the tiles b, b + wg.size(), ...) -- one workgroup's share unless the data is tied.  A launch whose list
// overflows (massively tied data: whole tiles within delta of the maximum) is repeated on fewer tiles -- one tile holds 16384
// pairs, so the halving ends -- and the tied tiles end up evaluated wholly in dist()'s arithmetic.
static const i64 NT_CAP = (i64)1 << 20;
template <class Flush>
static void dm_collect(cge_ctx *c, const double *Xs, const double *rns, i64 ld, i64 nrows, i64 dpad, const std::vector<int2> &tl,
                       int tri, double thr, const i32 *ids, Flush flush) {
    const i64 ntiles = (i64)tl.size();
    if (ntiles == 0) return;
    c->nt_pairs.ensure((size_t)NT_CAP);
    c->nt_tiles.ensure((size_t)ntiles);
    HIP_CHECK(hipMemcpyAsync(c->nt_tiles.p, tl.data(), sizeof(int2) * ntiles, hipMemcpyHostToDevice, c->stream));
    std::vector<int2> h;
    i64 t0 = 0, step = std::min<i64>(ntiles, (i64)1 << 17); // (a launch counts its pairs in 32 bits)
    while (t0 < ntiles) {
        const i64 t1 = std::min(ntiles, t0 + step);
        const i64 cnt = k_pair_collect(c, Xs, rns, ld, nrows, dpad, c->nt_tiles.p, t0, t1, tri, thr, ids, c->nt_pairs.p, NT_CAP);
        if (cnt > NT_CAP) {
            if (t1 - t0 <= 1) CGE_THROW(CGE_E_ARG, "diameter: a tile with more pairs than it has entries");
            step = (t1 - t0 + 1) / 2;
            continue;
        }
        if (cnt > 0) {
            h.resize(cnt);
            HIP_CHECK(hipMemcpyAsync(h.data(), c->nt_pairs.p, sizeof(int2) * cnt, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
            flush(h.data(), cnt);
        }
        t0 = t1;
    }
}

static void ensure_centred(cge_ctx *c) {
    if (c->centred_ready) return;
    if (c->rows_sharded) CGE_THROW(CGE_E_ARG, "the brute-force diameter over the whole embedding needs every row on one rank; the resident rows are sharded (option shard_rows)");
    if (!c->Xr.p || c->d <= 0) CGE_THROW(CGE_E_ARG, "diameter: embedding not resident");
    c->Xc.alloc_exact((size_t)c->ldn * c->dpad);
    c->rnorm.alloc_exact((size_t)c->ldn);
    k_gather_centre_fm(c, c->Xr.p, nullptr, c->gmean.p, c->Xc.p, c->rnorm.p, c->n, c->d, c->ldn, c->dpad);
    c->centred_ready = true;
}
void host_ensure_centred(cge_ctx *c) { ensure_centred(c); } // (the link model's top-k reads the same operands: link_host.cpp)

// Brute force over this rank's share of the pair tiles.  The arg-max launch leaves the largest Gram value `bv` of the shard's
// tiles and the workgroups' own (bv negative: the shard holds no pair); the pairs within rounding of it are evaluated with
// dist()'s own arithmetic (src/auxilary.jl:14-20) and the largest of THOSE values is `hi` (gram_delta).
double host_diameter_brute(cge_ctx *c, int part, int nparts, i64 *ai, i64 *aj) {
    ExactBest eb;
    if (c->emb_nonfinite) // (embedding_host.cpp: embedding_resident)
        eb.hi = std::numeric_limits<double>::quiet_NaN(); // as the reference's extrema()
    else {
        ensure_centred(c);
        double bv;
        i64 bi, bj;
        std::vector<double> wg;
        k_max_pair(c, c->Xc.p, c->rnorm.p, c->n, c->ldn, c->dpad, part, nparts, &bv, &bi, &bj, &wg);
        if (bv > -1.0) { // (identical rows can leave a Gram value a rounding below zero; -1 is "no pair")
            double rmax = 0.0;
            k_argmax_mapped(c, c->rnorm.p, c->n, nullptr, &rmax);
            const double thr = bv - gram_delta(c->dpad, rmax);
            std::vector<int2> tl;
            k_max_pair_tile_list(c->ldn, part, nparts, wg, thr, tl);
            dm_collect(c, c->Xc.p, c->rnorm.p, c->ldn, c->n, c->dpad, tl, 1, thr, nullptr,
                       [&](const int2 *p, i64 cnt) { dm_eval_pairs(c, p, cnt, eb); });
        }
        if (eb.hi < 0.0) eb.hi = 0.0; // (no pair: vertex 1 with itself)
    }
    c->stat_diameter_path = 1;
    c->stat_hi_i = eb.i; c->stat_hi_j = eb.j;
    if (ai) *ai = eb.i + 1;
    if (aj) *aj = eb.j + 1;
    return eb.hi;
}

// What the bound pass reads, left on the device by dm_prepare: the landmark-sorted layout, the reference points, the gathered
// operands of the pass the fitness verdict settled on, the row norms and the seed of the farthest-point sweep.
struct DmPrep {
    std::vector<i64> soff; // landmark a owns the sorted positions [soff[a], soff[a + 1])
    i64 npos = 0, lds_rows = 0;
    const i32 *d_off = nullptr, *d_mem = nullptr; // the landmark index on the device
    bool by_comm = false;                         // reference points: community centroids (else the landmark centroids)
    i64 nref = 0, ldm = 0, KP = 0;
    const double *mu_ref = nullptr;
    bool b16 = false, f32 = false; // the pass that runs (neither: fp64)
    double seed_norm = -1.0;
    i64 seed_vertex = -1;
};

// layout, reference points, gather and the fitness verdict of the low-precision passes (host_diameter_pruned's first stage,
// shared with the kernel-level testing hook); returns false when there are no member lists on the host
static bool dm_prepare(cge_ctx *c, const double *mu, const double *lw, const std::vector<i32> &lcomm, i64 C, i64 N,
                       const std::vector<i32> &mem_off, const std::vector<i32> &mem, DmPrep &S,
                       const std::function<void(const char *)> &lap) {
    const i64 n = c->n, d = c->d, dpad = c->dpad;
    const bool RS = c->rows_sharded;
    hipStream_t st = c->stream;
    // ---- landmark-sorted layout: landmark a owns positions [soff[a], soff[a] + cnt16[a]) (this rank's members) ------------
    std::vector<i64> &soff = S.soff;
    soff.assign(N + 1, 0);
    for (i64 a = 0; a < N; a++) soff[a + 1] = soff[a] + ((mem_off[a + 1] - mem_off[a] + 15) / 16) * 16;
    const i64 npos = S.npos = soff[N];
    const i64 lds_rows = S.lds_rows = (npos + 127) / 128 * 128 + 128;
    c->pos2node.ensure(std::max<i64>(npos, 1));
    c->sub_land.ensure(lds_rows / 16);
    const i32 *&d_off = S.d_off, *&d_mem = S.d_mem;
    d_off = c->lm_memoff.p;
    d_mem = c->lm_mem.p;
    {
        std::vector<i32> soff32(soff.begin(), soff.end());
        c->dm_soff.ensure(N + 1);
        WordPacker pk(c); // (small tables: one pinned staging buffer, no copy from pageable memory, no synchronisation for the local)
        pk.add(c->dm_soff.p, soff32.data(), N + 1);
        pk.flush();
        if (!(c->lm_index_on_device && mem_off.data() == c->h_mem_off.data())) {
            // index not produced by the landmark phase of this context (exact-mode callers): upload it
            if ((i64)mem.size() != n) return false; // no member lists on the host: the caller takes the brute-force path
            c->dm_memoff.ensure(N + 1);
            c->dm_mem.ensure(n);
            HIP_CHECK(hipMemcpyAsync(c->dm_memoff.p, mem_off.data(), sizeof(i32) * (N + 1), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(c->dm_mem.p, mem.data(), sizeof(i32) * n, hipMemcpyHostToDevice, st));
            d_off = c->dm_memoff.p;
            d_mem = c->dm_mem.p;
        }
        k_diameter_layout(c, d_off, d_mem, c->dm_soff.p, N, c->pos2node.p, c->sub_land.p, lds_rows / 16);
        if (d_off == c->dm_memoff.p) HIP_CHECK(hipStreamSynchronize(st)); // (the caller's index was copied from pageable memory)
    }
    lap("dm_layout");
    // ---- reference points ---------------------------------------------------------------------------------
    const bool by_comm = S.by_comm = C >= 32 && (i64)lcomm.size() == N && lw != nullptr;
    const i64 nref = S.nref = by_comm ? C : N;
    c->stat_nref = nref;
    std::vector<i32> lref(N);
    const double *&mu_ref = S.mu_ref;
    mu_ref = mu;
    if (by_comm) {
        std::vector<i32> roff(C + 1, 0), rmem(N);
        for (i64 a = 0; a < N; a++) {
            if (lcomm[a] < 0 || lcomm[a] >= C) CGE_THROW(CGE_E_ARG, "diameter: landmark community out of range");
            lref[a] = lcomm[a];
            roff[lcomm[a] + 1]++;
        }
        for (i64 q = 0; q < C; q++) roff[q + 1] += roff[q];
        std::vector<i32> cur(roff.begin(), roff.end() - 1);
        for (i64 a = 0; a < N; a++) rmem[cur[lcomm[a]]++] = (i32)a;
        c->mp_refoff.ensure(C + 1);
        c->mp_refmem.ensure(N);
        c->mp_refmu.ensure((size_t)C * d);
        c->mp_lref.ensure(N);
        WordPacker pk(c);
        pk.add(c->mp_refoff.p, roff.data(), C + 1);
        pk.add(c->mp_refmem.p, rmem.data(), N);
        pk.add(c->mp_lref.p, lref.data(), N);
        pk.flush();
        k_ref_centroids(c, mu, lw, c->mp_refoff.p, c->mp_refmem.p, C, d, c->mp_refmu.p);
        mu_ref = c->mp_refmu.p;
    } else {
        for (i64 a = 0; a < N; a++) lref[a] = (i32)a;
        c->mp_lref.ensure(N);
        WordPacker pk(c);
        pk.add(c->mp_lref.p, lref.data(), N);
        pk.flush();
    }
    const i64 ldm = S.ldm = (nref + 127) / 128 * 128;
    c->rns.ensure(lds_rows);
    c->Ms.ensure((size_t)ldm * dpad);
    c->mnorm.ensure(ldm);
    c->Pm.ensure((size_t)N * nref);
    // the maxima as upper bounds from a low-precision matrix pass (kernels_dist.hip (2b), (2c)) or exactly in fp64
    bool &b16 = S.b16, &f32 = S.f32;
    b16 = c->opt_diameter_f32 >= 2 && k_pcent_bf16_applies(dpad);
    f32 = c->opt_diameter_f32 != 0 && !b16;
    const i64 KP = S.KP = (dpad + 31) / 32 * 32;
    if (f32) {
        c->Xs32.ensure((size_t)lds_rows * dpad);
        c->Ms32.ensure((size_t)ldm * dpad);
    }
    if (b16) {
        c->Xb16.ensure((size_t)2 * lds_rows * KP);
        c->Mb16.ensure((size_t)2 * ldm * KP);
    }
    const bool lowp = b16 || f32;
    if (lowp) {
        c->dm_flag.ensure(1);
        HIP_CHECK(hipMemsetAsync(c->dm_flag.p, 0, sizeof(int), st));
    } else
        c->Xs.ensure((size_t)lds_rows * dpad);
    // the landmark-sorted rows: norms + the operands of the bound pass.  The fp64 feature-major copy is written only when the
    // bound pass itself is fp64 (the exact stage gathers what it needs, below)
    k_gather_centre_fm(c, c->Xr.p, c->pos2node.p, c->gmean.p, lowp ? nullptr : c->Xs.p, c->rns.p, npos, d, lds_rows, dpad,
                       f32 ? c->Xs32.p : nullptr, b16 ? c->Xb16.p : nullptr, KP, lowp ? c->dm_flag.p : nullptr);
    k_gather_centre_fm(c, mu_ref, nullptr, c->gmean.p, c->Ms.p, c->mnorm.p, nref, d, ldm, dpad, f32 ? c->Ms32.p : nullptr,
                       b16 ? c->Mb16.p : nullptr, KP, lowp ? c->dm_flag.p : nullptr);
    int unfit = 0;
    if (lowp) HIP_CHECK(hipMemcpyAsync(&unfit, c->dm_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    // the seed of the farthest-point sweep: the vertex farthest from the centre (largest squared norm of the centred rows, just
    // computed by the gather); its read-back is the synchronisation the flag needs anyway
    S.seed_norm = -1.0;
    S.seed_vertex = k_argmax_mapped(c, c->rns.p, npos, c->pos2node.p, &S.seed_norm); // (a row id of this rank)
    // The exact fp64 pass (below) instead of a low-precision one when a centred value lies beyond 2^+-100 or is not finite
    // (bit 0), or when NO centred value reaches 2^-40 (bit 1 clear): products below 2^-126 are flushed to zero in the fp32
    // accumulators, an absolute error of < 3K 2^-126 per dot product that the relative margin e only covers while the
    // distances that matter (>= L >= the largest centred norm squared >= 2^-80) dwarf it.
    if (RS && lowp) {
        // option shard_rows: the verdict is taken TOGETHER -- "some rank holds an unfit value" (max of bit 0) and "some
        // rank holds a value of normal size" (max of bit 1) -- so every rank runs the same bound pass whatever rows it happens
        // to hold (a rank without rows of its own simply agrees): the candidate set, the statistics and the timing no longer
        // depend on the sharding
        const double bad = cge_allreduce_scalar_max(c, (unfit & 1) ? 1.0 : 0.0), big = cge_allreduce_scalar_max(c, (unfit & 2) ? 1.0 : 0.0);
        unfit = (bad != 0.0 ? 1 : 0) | (big != 0.0 ? 2 : 0);
    }
    if (lowp && ((unfit & 1) || !(unfit & 2))) {
        b16 = f32 = false;
        c->Xs.ensure((size_t)lds_rows * dpad);
        k_gather_centre_fm(c, c->Xr.p, c->pos2node.p, c->gmean.p, c->Xs.p, c->rns.p, npos, d, lds_rows, dpad, nullptr, nullptr, KP, nullptr);
    }
    c->stat_bound_pass = b16 ? 2 : (f32 ? 1 : 0);
    return true;
}

// the bound pass dm_prepare settled on: c->Pm (N x nref) = upper bounds of max_{i in a} ||x_i - ref_r||^2
static void dm_bound_pass(cge_ctx *c, const DmPrep &S, i64 N, int part, int nparts) {
    const i64 dpad = c->dpad;
    if (S.npos > 0) {
        if (S.b16)
            k_pcent_bf16(c, c->Xb16.p, c->rns.p, S.lds_rows, c->Mb16.p, c->mnorm.p, S.ldm, N, S.nref, S.KP, c->sub_land.p, c->Pm.p, part, nparts);
        else if (S.f32)
            k_pcent_f32(c, c->Xs32.p, c->rns.p, S.lds_rows, c->Ms32.p, c->mnorm.p, S.ldm, N, S.nref, dpad, c->dm_soff.p, c->Pm.p, part, nparts);
        else
            k_pcent(c, c->Xs.p, c->rns.p, S.lds_rows, c->Ms.p, c->mnorm.p, S.ldm, N, S.nref, dpad, c->sub_land.p, c->Pm.p, part, nparts);
    } else
        HIP_CHECK(hipMemsetAsync(c->Pm.p, 0, sizeof(double) * (size_t)(N * S.nref), c->stream));
}

// ---- the pruned search: what its stages share ------------------------------------------------------------------------------
// `mu` = N landmark centroids (device, row-major), `lw` their weights (device) and `lcomm` their communities (host, 0-based, C
// communities).  Reference points: the community centroids when there are at least 32 communities (the MFMA pass is then
// n*C*d instead of n*N*d), else the landmark centroids themselves.
//
// THE EXACT STAGE WORKS ON GATHERED ROWS: no fp64 copy of the whole landmark-sorted embedding is written; the few landmarks that
// survive the bounds are gathered per round -- centred, feature-major, fp64 -- into `xe`, and the tile kernel runs on that.
//
// OPTION shard_rows (c->rows_sharded): `mem_off` / the device index hold THIS RANK's members (local row ids, other ranks'
// landmarks are empty ranges), c->h_gl_off the global sizes.  Every rank bounds its own rows (all-reduce(max) of the bound
// matrix), the seed row of the farthest-point sweep is fetched from its owner, and the gathered rows of a round are
// completed by an all-reduce of the zero-filled gather (op 2: exact), so a candidate pair whose landmarks live on two ranks
// is evaluated like any other; the rounds are taken in lock-step (the best value so far is all-reduced after each).
struct DmSearch {
    cge_ctx *c;
    const bool RS;                  // option shard_rows ...
    const int W, me;                // ... and then the ranks that hold the rows, this one among them (else 1, 0)
    const int part, nparts;         // this rank's share of work on rows that every rank holds
    const i64 N;
    const std::vector<i32> &gl_off; // sizes of the WHOLE landmarks
    DmPrep prep;
    double rmax = -1.0;             // the largest squared norm of a centred row, of all ranks
    double L = 0.0;                 // the sweep's lower bound of the diameter^2 and its pair (global vertex ids; the seed first)
    i64 far_i = -1, far_j = -1;
    double delta = 0.0;             // gram_delta of this embedding
    ExactBest eb;
    double best = 0.0;              // a lower bound of the largest Gram value
    std::vector<BoundRec> cand;     // the candidate landmark pairs: a heap in [0, left), largest bound first
    size_t left = 0;
    double tphase = now_ms();
    void lap(const char *name) { const double t = now_ms(); c->phases.ms[name] += t - tphase; tphase = t; } // host wall time per stage
    i64 len16(i64 a) const { return (i64)((gl_off[a + 1] - gl_off[a] + 15) / 16 * 16); } // positions of the WHOLE landmark
    // the 128x128 tiles of a candidate pair: tile rows (x < ta) times tile columns (y < tb), of a landmark with itself those with y >= x
    i64 pair_tiles(const BoundRec &r, const std::function<void(i64, i64)> &visit = nullptr) const {
        const i64 ta = (len16(r.a) + 127) / 128, tb = (len16(r.b) + 127) / 128;
        if (visit)
            for (i64 x = 0; x < ta; x++)
                for (i64 y = (r.a == r.b ? x : 0); y < tb; y++) visit(x, y);
        return r.a == r.b ? ta * (ta + 1) / 2 : ta * tb;
    }
};
static bool cand_later(const BoundRec &x, const BoundRec &y) { // x comes after y: decreasing bound, ties by landmark pair
    return x.B < y.B || (x.B == y.B && (x.a > y.a || (x.a == y.a && x.b > y.b)));
}

// The lowest rank among those whose `v` is the largest of all ranks' wins (`can`: this rank may win); *vmax = that largest value.
// Collective: every rank of the shard_rows group calls it, and gets the same answer (world when nobody can win).
static int dm_elect(cge_ctx *c, double v, bool can, double *vmax) {
    const int W = c->coll.world, me = c->coll.rank;
    *vmax = cge_allreduce_scalar_max(c, v);
    const double claim = cge_allreduce_scalar_max(c, (v == *vmax && can) ? (double)(W - me) : 0.0);
    return W - (int)claim;
}

// One farthest-point sweep from the vertex farthest from the centre (a memory-bound read of Xr) and the reference points' mutual
// distances (candidate selection), enqueued on the side stream AHEAD of the bound pass: neither depends on it (the gathers that
// wrote Ms are done: the seed's read-back in dm_prepare synchronised the main stream).  Launched first, the sweep's small
// workgroups fill the CUs and it runs at its own speed (~0.3 ms) while the bound pass's one-workgroup-per-CU tiles move in
// beside them -- launched behind it, the sweep was left the gaps (1.0 ms, the longer of the two concurrent branches).
static void dm_seed_sweep(DmSearch &S) {
    cge_ctx *c = S.c;
    const DmPrep &P = S.prep;
    const i64 d = c->d;
    if (!S.RS) {
        S.far_i = S.far_j = P.seed_vertex;
        S.rmax = P.seed_norm;
        SideStream side(c);
        k_farthest_enqueue(c, c->Xr.p, c->n, d, P.seed_vertex);
        k_ref_dist2_fm(c, c->Ms.p, P.nref, c->dpad, P.ldm);
        return;
    }
    // option shard_rows: the seed is the farthest of ALL ranks' rows, its owner hands the row itself (and its vertex id) to
    // everybody; the sweep then runs over every rank's own rows on the main stream
    hipStream_t st = c->stream;
    const int winner = dm_elect(c, P.seed_norm, P.seed_vertex >= 0, &S.rmax);
    c->dm_seed.ensure(d + 1);
    HIP_CHECK(hipMemsetAsync(c->dm_seed.p, 0, sizeof(double) * (d + 1), st));
    if (winner == S.me) {
        HIP_CHECK(hipMemcpyAsync(c->dm_seed.p, c->Xr.p + P.seed_vertex * d, sizeof(double) * d, hipMemcpyDeviceToDevice, st));
        const double gid = (double)(c->h_loc2glob[P.seed_vertex] + 1);
        HIP_CHECK(hipMemcpyAsync(c->dm_seed.p + d, &gid, sizeof(double), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st)); // gid is a stack variable
    }
    cge_allreduce_dev(c, c->dm_seed.p, d + 1, 2);
    double gid = 0.0;
    HIP_CHECK(hipMemcpyAsync(&gid, c->dm_seed.p + d, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    S.far_i = S.far_j = (i64)gid - 1;
    k_farthest_enqueue(c, c->Xr.p, lm_rows(c), d, 0, c->dm_seed.p);
    k_ref_dist2_fm(c, c->Ms.p, P.nref, c->dpad, P.ldm);
}

// The bound pass (c->Pm) and the sweep's lower bound L.  The sweep left its result (a double and an id per workgroup) in
// c->mp_recs, scratch of the arg-max launches.  With shard_rows the sweep shares the main stream with everything else and its
// result is collected BEFORE the bound pass; without, it runs on the side stream and is collected AFTER the bound pass has been
// enqueued (the bound passes do not touch c->mp_recs): a collect in front would wait for the sweep with the bound pass not
// yet launched, and the overlap the sweep was launched ahead for would be gone.
static void dm_bounds(DmSearch &S) {
    cge_ctx *c = S.c;
    const DmPrep &P = S.prep;
    double v = -1.0, Lmax;
    i64 q = 0;
    if (S.RS) {
        k_farthest_collect(c, &v, &q);
        const int winner = dm_elect(c, v, true, &Lmax);
        const double qid = cge_allreduce_scalar_max(c, winner == S.me ? (double)(c->h_loc2glob[q] + 1) : 0.0);
        if (Lmax > S.L) { S.L = Lmax; S.far_j = (i64)qid - 1; }
    }
    // P is a maximum over vertices: with several ranks each takes its share of the vertex tiles (all of its own rows when the
    // rows are sharded) and the maxima are combined by one all-reduce(max)
    const bool shard_q = !S.RS && S.nparts > 1 && c->has_coll && (c->rccl_comm || (c->xptr && (size_t)(S.N * P.nref) <= c->xcap));
    dm_bound_pass(c, P, S.N, shard_q ? S.part : 0, shard_q ? S.nparts : 1);
    if (shard_q || S.RS) cge_allreduce_dev(c, c->Pm.p, S.N * P.nref, 1);
    S.lap("dm_refs_pcent");
    if (!S.RS) {
        SideStream side(c);
        k_farthest_collect(c, &v, &q);
        if (v > S.L) { S.L = v; S.far_j = q; }
    }
    S.lap("dm_farthest");
}

// The candidate landmark pairs: those whose bound reaches L, as a heap.  Returns false when the bounds prune too little.
// The sweep's L is a distance in a THIRD arithmetic (16 partial sums per row): it enters the search as a bound on the Gram
// values, delta below itself (gram_delta: eta covers any summation order), and its pair as the first evaluated candidate.
// The selection here and the stop test of the rounds compare bounds with relative margins of 1e-9 on either side: with
// rmax <= L (the seed is the row farthest from the centre, and some row lies at least that far from it) delta is below
// 2e-12 L for every d <= 512, so those margins already leave delta of room a hundred times over.
static bool dm_select(DmSearch &S) {
    cge_ctx *c = S.c;
    const DmPrep &P = S.prep;
    S.delta = gram_delta(c->dpad, std::max(S.rmax, 0.0));
    const int2 far = make_int2((int)S.far_i, (int)S.far_j);
    dm_eval_pairs(c, &far, 1, S.eb);
    const i64 cap = std::min<i64>(S.N * (S.N + 1) / 2, (i64)4 << 20);
    c->bound_list.ensure((size_t)cap);
    const i64 cnt = k_bound_select(c, c->Pm.p, c->mp_lref.p, S.N, P.nref, S.L * (1.0 - 1e-9), c->bound_list.p, cap,
                                   P.by_comm ? c->mp_refoff.p : nullptr, P.by_comm ? c->mp_refmem.p : nullptr);
    c->stat_cand_pairs = cnt;
    if (cnt > cap) {
        if (S.RS) CGE_THROW(CGE_E_ARG, "diameter (shard_rows): the bounds prune too little (more than %lld candidate landmark pairs) and the brute-force "
                                       "fallback needs every row on one rank", (long long)cap);
        return false;
    }
    S.cand.resize(cnt);
    if (cnt > 0) {
        HIP_CHECK(hipMemcpyAsync(S.cand.data(), c->bound_list.p, sizeof(BoundRec) * cnt, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    S.lap("dm_select");
    // candidates are consumed in decreasing-bound order (ties: by landmark pair) until the bound drops below the best
    // pair found: a heap delivers exactly that order without sorting the (mostly never visited) tail
    std::make_heap(S.cand.begin(), S.cand.end(), cand_later);
    S.left = S.cand.size();
    double tiles_total = 0.0;
    for (const BoundRec &r : S.cand) tiles_total += (double)S.pair_tiles(r);
    const double nT = (double)((c->n + 127) / 128);
    if (!S.RS && c->opt_diameter != 2 && tiles_total > 0.5 * nT * (nT + 1) / 2) return false; // pruning too weak: brute force
    S.best = S.L - S.delta; // the farthest-point pair is a valid answer so far
    return true;
}

// A round of the exact evaluation: the next candidates, as many as fit the tile and row budgets, on the gathered rows of their landmarks
struct DmRound {
    std::vector<BoundRec> pairs;
    std::vector<i32> lms;       // its landmarks ...
    std::vector<char> in_round; // ... as flags (all clear between rounds)
    std::vector<i32> eoff;      // landmark a owns the positions [eoff[a], eoff[a + 1]) of the round (outside the round: none)
    i64 E = 0, ldE = 0;         // positions / the row stride of xe
    i64 tile_cap = 4096;        // the first round is short: it usually raises `best` past most of the candidates
    i64 global_tile = 0;        // tiles so far: tile t is evaluated by rank t % (ranks)
    explicit DmRound(i64 N) : in_round(N, 0), eoff(N + 1) {}
};

// pops the round's pairs off the heap; false: nothing left that can win
static bool dm_round_fill(DmSearch &S, DmRound &R) {
    const i64 pos_cap = std::max<i64>(8192, ((i64)512 << 20) / (S.c->dpad * 8)); // <= 512 MB of gathered rows per round
    std::vector<BoundRec> &cand = S.cand;
    R.pairs.clear();
    R.lms.clear();
    R.E = 0;
    i64 ntile = 0;
    while (S.left > 0 && ntile < R.tile_cap) {
        std::pop_heap(cand.begin(), cand.begin() + S.left, cand_later);
        const BoundRec r = cand[S.left - 1];
        if (r.B * (1.0 + 1e-9) + 1e-9 < S.best) { S.left = 0; break; } // decreasing order: nothing further can win
        const i64 extra = (R.in_round[r.a] ? 0 : S.len16(r.a)) + ((r.b != r.a && !R.in_round[r.b]) ? S.len16(r.b) : 0);
        if (!R.pairs.empty() && R.E + extra > pos_cap) { // the round is full: the pair goes back, the next round takes it
            std::push_heap(cand.begin(), cand.begin() + S.left, cand_later);
            break;
        }
        S.left--;
        R.pairs.push_back(r);
        for (i32 a : {r.a, r.b})
            if (!R.in_round[a]) { R.in_round[a] = 1; R.lms.push_back(a); R.E += S.len16(a); }
        ntile += S.pair_tiles(r);
    }
    R.tile_cap = 131072;
    return !R.pairs.empty();
}

// positions of the round -- its landmarks in ascending id, each padded to 16 -- and their rows: centred, feature-major, with
// norms and vertex ids
static void dm_round_gather(DmSearch &S, DmRound &R) {
    cge_ctx *c = S.c;
    const i64 N = S.N, d = c->d, dpad = c->dpad, E = R.E;
    i64 at = 0;
    for (i64 a = 0; a < N; a++) {
        R.eoff[a] = (i32)at;
        if (R.in_round[a]) at += S.len16(a);
    }
    R.eoff[N] = (i32)at;
    for (i32 a : R.lms) R.in_round[a] = 0;
    const i64 ldE = R.ldE = (E + 127) / 128 * 128 + 128;
    c->dm_soffE.ensure(N + 1); c->xe_pos.ensure(E); c->xe_glob.ensure(E + 2); c->xe_sub.ensure(ldE / 16);
    c->xe.ensure((size_t)ldE * dpad); c->xe_rns.ensure(ldE);
    WordPacker pk(c);
    pk.add(c->dm_soffE.p, R.eoff.data(), N + 1);
    pk.flush();
    k_diameter_layout(c, S.prep.d_off, S.prep.d_mem, c->dm_soffE.p, N, c->xe_pos.p, c->xe_sub.p, ldE / 16);
    k_gather_centre_fm(c, c->Xr.p, c->xe_pos.p, c->gmean.p, c->xe.p, c->xe_rns.p, E, d, ldE, dpad);
    k_position_ids(c, c->xe_pos.p, S.RS ? c->loc2glob.p : nullptr, E, c->xe_glob.p);
    if (S.RS) { // every rank has filled the rows it owns: the ranks add the words (zeros elsewhere: exact)
        HIP_CHECK(hipMemsetAsync(c->xe_glob.p + E, 0, sizeof(i32) * 2, c->stream));
        cge_allreduce_dev(c, c->xe.p, ldE * dpad, 2);
        cge_allreduce_dev(c, c->xe_rns.p, ldE, 2);
        cge_allreduce_dev(c, reinterpret_cast<double *>(c->xe_glob.p), (E + 1) / 2, 2);
    }
}

// this rank's tiles of the round through the arg-max kernel; when the round's best Gram value comes within delta of the best
// so far, its near-ties are collected and their dist() values decide
static void dm_round_eval(DmSearch &S, DmRound &R) {
    cge_ctx *c = S.c;
    const int xparts = S.RS ? S.W : S.nparts, xpart = S.RS ? S.me : S.part; // who evaluates which tile
    std::vector<int2> tiles, near, pool; // this rank's tiles / those that can hold a near-tie / (shard_rows) its near-ties, pooled with the other ranks'
    std::vector<double> wg_best;         // the best Gram value of each workgroup of the arg-max launch
    for (const BoundRec &r : R.pairs)
        S.pair_tiles(r, [&](i64 x, i64 y) {
            if ((R.global_tile++ % xparts) == xpart) tiles.push_back(make_int2((int)(R.eoff[r.a] + 128 * x), (int)(R.eoff[r.b] + 128 * y)));
        });
    double v = -1.0;
    if (!tiles.empty()) {
        c->stat_cand_tiles += (i64)tiles.size();
        c->tile_list.ensure(tiles.size());
        WordPacker pk(c);
        pk.add(c->tile_list.p, tiles.data(), (i64)tiles.size());
        pk.flush();
        i64 pi, pj;
        k_pair_list(c, c->xe.p, c->xe_rns.p, R.ldE, R.E, c->dpad, c->tile_list.p, (i64)tiles.size(), &v, &pi, &pj, &wg_best);
    }
    if (S.RS) v = cge_allreduce_scalar_max(c, v); // the rounds are taken in lock-step with one threshold
    if (v > S.best) S.best = v;
    const double thr = S.best - S.delta;
    if (!(v >= thr)) return; // else the round holds pairs that may carry the maximum
    for (size_t t = 0; t < tiles.size(); t++)
        if (wg_best[t % wg_best.size()] >= thr) near.push_back(tiles[t]);
    dm_collect(c, c->xe.p, c->xe_rns.p, R.ldE, R.E, c->dpad, near, 0, thr, c->xe_glob.p, [&](const int2 *p, i64 cnt) {
        if (S.RS) pool.insert(pool.end(), p, p + cnt);
        else dm_eval_pairs(c, p, cnt, S.eb);
    });
    if (S.RS) dm_eval_pairs(c, pool.data(), (i64)pool.size(), S.eb);
}

// returns false when the caller should fall back to brute force
// (the landmark index is the one this context's landmark phase left: c->h_mem_off / c->h_mem)
static bool host_diameter_pruned(cge_ctx *c, const double *mu, const double *lw, const std::vector<i32> &lcomm, i64 C, i64 N,
                                 int part, int nparts, ExactBest &eb) {
    const bool RS = c->rows_sharded;
    c->stat_cand_pairs = c->stat_cand_tiles = 0;
    if (RS && ((i64)c->h_gl_off.size() != N + 1 || !c->lm_index_on_device))
        CGE_THROW(CGE_E_ARG, "diameter (shard_rows): the landmark index of this context's own landmark phase is required");
    DmSearch S{c, RS, RS ? c->coll.world : 1, RS ? c->coll.rank : 0, part, nparts, N, RS ? c->h_gl_off : c->h_mem_off};
    if (!dm_prepare(c, mu, lw, lcomm, C, N, c->h_mem_off, c->h_mem, S.prep, [&](const char *name) { S.lap(name); })) return false;
    dm_seed_sweep(S);
    dm_bounds(S);
    if (!dm_select(S)) return false;
    DmRound R(N);
    while (dm_round_fill(S, R)) {
        dm_round_gather(S, R);
        dm_round_eval(S, R);
    }
    S.lap("dm_exact");
    eb = S.eb;
    return true;
}

// The diameter of a score, full_graph_D's normaliser (src/divergence.jl:104-114): the largest of the ranks' shares.  Brute force when
// the option asks for it, without a landmark index, or when the bounds prune too little (sharded rows: the pruned search only).
double host_diameter_landmarks(cge_ctx *c, const double *lemb, const double *lweight, const std::vector<i32> &lcomm, i64 C, i64 N) {
    const int part = c->has_coll ? c->coll.rank : 0, nparts = c->has_coll ? c->coll.world : 1;
    ExactBest eb;
    if (!c->emb_nonfinite && (c->opt_diameter != 1 || c->rows_sharded) && (i64)c->h_mem_off.size() == N + 1 &&
        host_diameter_pruned(c, lemb, lweight, lcomm, C, N, part, nparts, eb)) {
        c->stat_diameter_path = 2;
        c->stat_hi_i = eb.i; c->stat_hi_j = eb.j;
    } else
        eb.hi = host_diameter_brute(c, part, nparts, nullptr, nullptr);
    const double hi = cge_allreduce_scalar_max(c, eb.hi);
    c->stat_last_hi = hi;
    return hi;
}

// Testing hook (include/cge_hip_testing.h: cge_diameter_bounds_test): dm_prepare and dm_bound_pass -- the same launch wrappers
// as host_diameter_pruned, in the same order -- on the resident embedding for a caller-supplied landmark assignment.  The
// landmarks' centroids (the plain mean of their members, weight = their size) are formed on the host.
void host_diameter_bounds_test(cge_ctx *c, const i64 *v2l, i64 N, const i64 *lcomm1, i64 C, int pass, double *P, i64 *nref_out,
                               int *pass_ran, double *ref_out, double *mean_out) {
    const i64 n = c->n, d = c->d;
    if (!c->Xr.p || n <= 0 || d <= 0) CGE_THROW(CGE_E_ARG, "diameter bounds: embedding not resident");
    if (c->rows_sharded) CGE_THROW(CGE_E_ARG, "diameter bounds: the testing hook needs every row on one rank");
    if (pass == 2 && !k_pcent_bf16_applies(c->dpad)) CGE_THROW(CGE_E_ARG, "diameter bounds: the bf16 split pass needs d <= 128");
    hipStream_t st = c->stream;
    std::vector<i32> mem_off(N + 1, 0), mem(n), lc(N);
    for (i64 i = 0; i < n; i++) {
        if (v2l[i] < 1 || v2l[i] > N) CGE_THROW(CGE_E_ARG, "diameter bounds: landmark id %lld outside 1..%lld", (long long)v2l[i], (long long)N);
        mem_off[v2l[i]]++;
    }
    for (i64 a = 0; a < N; a++) {
        if (mem_off[a + 1] == 0) CGE_THROW(CGE_E_ARG, "diameter bounds: landmark %lld has no member", (long long)(a + 1));
        if (lcomm1[a] < 1 || lcomm1[a] > C) CGE_THROW(CGE_E_ARG, "diameter bounds: community %lld outside 1..%lld", (long long)lcomm1[a], (long long)C);
        lc[a] = (i32)(lcomm1[a] - 1);
        mem_off[a + 1] += mem_off[a];
    }
    {
        std::vector<char> seen(C, 0);
        for (i64 a = 0; a < N; a++) seen[lc[a]] = 1;
        for (i64 q = 0; q < C; q++)
            if (!seen[q]) CGE_THROW(CGE_E_ARG, "diameter bounds: community %lld has no landmark", (long long)(q + 1));
    }
    {
        std::vector<i32> cur(mem_off.begin(), mem_off.end() - 1);
        for (i64 i = 0; i < n; i++) mem[cur[v2l[i] - 1]++] = (i32)i;
    }
    std::vector<double> X((size_t)n * d), mu((size_t)N * d, 0.0), lw(N);
    HIP_CHECK(hipMemcpyAsync(X.data(), c->Xr.p, sizeof(double) * n * d, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (i64 a = 0; a < N; a++) {
        const i64 cnt = mem_off[a + 1] - mem_off[a];
        lw[a] = (double)cnt;
        for (i64 q = mem_off[a]; q < mem_off[a + 1]; q++)
            for (i64 k = 0; k < d; k++) mu[a * d + k] += X[(i64)mem[q] * d + k];
        for (i64 k = 0; k < d; k++) mu[a * d + k] /= (double)cnt;
    }
    DevBuf<double> dmu, dlw;
    dmu.ensure((size_t)N * d);
    dlw.ensure(N);
    HIP_CHECK(hipMemcpyAsync(dmu.p, mu.data(), sizeof(double) * N * d, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dlw.p, lw.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    struct KeepOption { int &ref; int val; ~KeepOption() { ref = val; } } keep{c->opt_diameter_f32, c->opt_diameter_f32};
    c->opt_diameter_f32 = pass;
    DmPrep S;
    if (!dm_prepare(c, dmu.p, dlw.p, lc, C, N, mem_off, mem, S, [](const char *) {}))
        CGE_THROW(CGE_E_ARG, "diameter bounds: no landmark index");
    dm_bound_pass(c, S, N, 0, 1);
    HIP_CHECK(hipMemcpyAsync(P, c->Pm.p, sizeof(double) * (size_t)(N * S.nref), hipMemcpyDeviceToHost, st));
    if (ref_out) HIP_CHECK(hipMemcpyAsync(ref_out, S.mu_ref, sizeof(double) * (size_t)(S.nref * d), hipMemcpyDeviceToHost, st));
    if (mean_out) HIP_CHECK(hipMemcpyAsync(mean_out, c->gmean.p, sizeof(double) * d, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    *nref_out = S.nref;
    *pass_ran = c->stat_bound_pass;
}

// Testing hook (include/cge_hip_testing.h: cge_ref_dist2_test): the reference points' mutual squared distances for caller-supplied
// rows -- the gather of dm_prepare's reference operand (centred with the resident embedding's mean, feature-major, fp64), then
// the launch wrapper dm_seed_sweep uses.
void host_ref_dist2_test(cge_ctx *c, const double *refs, i64 nref, double *rd2, double *mean_out) {
    const i64 d = c->d, dpad = c->dpad;
    if (!c->Xr.p || c->n <= 0 || d <= 0) CGE_THROW(CGE_E_ARG, "reference distances: embedding not resident");
    hipStream_t st = c->stream;
    const i64 ldm = (nref + 127) / 128 * 128;
    DevBuf<double> dref;
    dref.ensure((size_t)nref * d);
    HIP_CHECK(hipMemcpyAsync(dref.p, refs, sizeof(double) * nref * d, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    c->Ms.ensure((size_t)ldm * dpad);
    c->mnorm.ensure(ldm);
    k_gather_centre_fm(c, dref.p, nullptr, c->gmean.p, c->Ms.p, c->mnorm.p, nref, d, ldm, dpad, nullptr, nullptr, (dpad + 31) / 32 * 32, nullptr);
    k_ref_dist2_fm(c, c->Ms.p, nref, dpad, ldm);
    HIP_CHECK(hipMemcpyAsync(rd2, c->mp_rd2.p, sizeof(double) * (size_t)(nref * nref), hipMemcpyDeviceToHost, st));
    if (mean_out) HIP_CHECK(hipMemcpyAsync(mean_out, c->gmean.p, sizeof(double) * d, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}
