// common.hpp -- context, device buffers, error handling and launch helpers of libcge_hip.so.
// gfx950 (MI355X) only; there is no CPU fallback anywhere in this library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cge_hip.h"

typedef int64_t i64;
typedef int32_t i32;

// records the diameter's kernels (kernels_dist.hip) write and its host code (diameter_host.cpp) reads
struct MaxRec { // a workgroup's best: value max, ties -> smallest (i, j)
    double val;
    i64 i, j;
};
struct BoundRec { // a candidate landmark pair a <= b and the upper bound of its pairs' squared distances
    double B;
    i32 a, b;
};

struct CgeError {
    int code;
    std::string msg;
};

#define CGE_THROW(code, ...)                                  \
    do {                                                      \
        char _b[512];                                         \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                \
        throw CgeError{(code), std::string(_b)};              \
    } while (0)

#define HIP_CHECK(expr)                                                                                 \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            CGE_THROW(_e == hipErrorOutOfMemory ? CGE_E_OOM : CGE_E_HIP, "%s failed: %s (%s:%d)", #expr, \
                      hipGetErrorString(_e), __FILE__, __LINE__);                                       \
    } while (0)

// the body of an extern "C" entry point: an exception becomes the context's message and a status
#define CGE_TRY(ctx) try {
#define CGE_TRY_ON_DEVICE(ctx) CGE_TRY(ctx) HIP_CHECK(hipSetDevice((ctx)->device)); // ... on the context's device
#define CGE_CATCH(ctx)                                             \
    }                                                              \
    catch (const CgeError &e) {                                    \
        if (ctx) (ctx)->err = e.msg;                               \
        return e.code;                                             \
    }                                                              \
    catch (const std::bad_alloc &) {                               \
        if (ctx) (ctx)->err = "host allocation failed";            \
        return CGE_E_OOM;                                          \
    }                                                              \
    catch (const std::exception &e) {                              \
        if (ctx) (ctx)->err = e.what();                            \
        return CGE_E_ARG;                                          \
    }                                                              \
    return CGE_OK;

// Every kernel launch of the library is followed by hipGetLastError: a refused launch (dynamic LDS beyond what the device
// grants, a bad grid) raises CGE_E_HIP instead of leaving the output at its memset zeros.
inline void cge_launch_check(const char *what, const char *file, int line) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) CGE_THROW(CGE_E_HIP, "launch of %s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...)                         \
    do {                                                            \
        hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__);      \
        cge_launch_check(#kernelName, __FILE__, __LINE__);          \
    } while (0)

// Dynamic LDS beyond 64 KB has to be granted per kernel AND per device (the attribute belongs to the function's code object on
// the current device); the grant is checked.
inline void cge_allow_lds(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> done;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(mu);
    auto it = done.find({fn, dev});
    if (it != done.end() && it->second >= bytes) return;
    HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[{fn, dev}] = bytes;
}

// RAII device buffer
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void swap(DevBuf &o) { // (ownership changes hands; the device pointers stay valid)
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
    // grow-only allocation (contents are NOT preserved)
    void ensure(size_t count) {
        if (count <= n && p) return;
        release();
        if (count == 0) count = 1;
        HIP_CHECK(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
    }
    void alloc_exact(size_t count) {
        release();
        HIP_CHECK(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
        n = count ? count : 1;
    }
};

// pinned (page-locked) host buffer, grow-only
template <typename T>
struct PinBuf {
    T *p = nullptr;
    size_t n = 0;
    PinBuf() {}
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    void ensure(size_t count) {
        if (count <= n && p) return;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        if (count == 0) count = 1;
        HIP_CHECK(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault));
        n = count;
    }
};

// Persistent worker pool: run(n, fn) executes fn(0..n-1) on the workers + the calling thread.
// Completion is counted in ITEMS, not in workers: the caller takes items itself and returns as soon as the last one is
// done, so a worker that is slow to wake up (a sleeping core: milliseconds, seen as sporadic 2-6 ms stalls of a 0.1 ms
// job) delays nobody -- it finds the job drained and goes back to sleep.
class ThreadPool {
  public:
    explicit ThreadPool(int n_workers) {
        for (int t = 0; t < n_workers; t++) workers_.emplace_back([this]() { loop(); });
    }
    ~ThreadPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
            gen_++;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    int size() const { return (int)workers_.size() + 1; }
    void run(i64 n, const std::function<void(i64)> &fn) {
        if (n <= 0) return;
        if (n == 1 || workers_.empty()) {
            for (i64 i = 0; i < n; i++) fn(i);
            return;
        }
        auto job = std::make_shared<Job>();
        job->fn = &fn;
        job->n = n;
        {
            std::lock_guard<std::mutex> lk(m_);
            cur_ = job;
            gen_++;
        }
        cv_.notify_all();
        work(*job);
        while (job->done.load(std::memory_order_acquire) < n) std::this_thread::yield(); // items other threads still hold
        // (a late worker may still look at `job` through its own reference: it finds next >= n and never touches fn)
    }

  private:
    struct Job {
        const std::function<void(i64)> *fn = nullptr;
        i64 n = 0;
        std::atomic<i64> next{0}, done{0};
    };
    static void work(Job &j) {
        for (;;) {
            const i64 i = j.next.fetch_add(1);
            if (i >= j.n) break;
            (*j.fn)(i);
            j.done.fetch_add(1, std::memory_order_release);
        }
    }
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            std::shared_ptr<Job> job;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&]() { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                job = cur_;
            }
            if (job) work(*job);
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_;
    std::shared_ptr<Job> cur_;
    unsigned long long gen_ = 0;
    bool stop_ = false;
};

struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    i64 launches = 0;
    double total_ms = 0.0;
};

struct Phase {
    std::map<std::string, double> ms;
};

// Device view of the graph that wGCL scores ("score graph": the landmark graph in landmark mode,
// the original graph in exact mode).  All ids 0-based on the device.
struct ScoreGraph {
    i64 N = 0, d = 0, C = 0;
    const double *emb = nullptr;   // N x d row-major
    const double *dist = nullptr;  // N   (diagonal of D: dii or zeros)
    const double *vw = nullptr;    // N   (Chung-Lu target weights; undirected)
    const i32 *comm = nullptr;     // N   0-based community
    const double *vectC = nullptr; // packed p(C) (undirected) or C*C (directed)
    const double *deg_in = nullptr, *deg_out = nullptr; // directed only
};

struct SampleSet {
    i64 S = 0, n_sets = 0;
    std::vector<i64> pos_idx, neg_i, neg_j, pos_idx2; // 1-based (caller-provided draws, small graphs)
    // library-drawn samples of a large resident graph stay on the device (0-based, n_sets * S each)
    bool on_device = false;
    DevBuf<i32> d_pos, d_ni, d_nj, d_pos2;
    void reset() { // the device buffers are grow-only scratch: they stay
        S = n_sets = 0;
        on_device = false;
        pos_idx.clear(); neg_i.clear(); neg_j.clear(); pos_idx2.clear();
    }
};
struct DevSamples { // one sample set as the AUC kernels read it (device, 0-based)
    DevBuf<i32> pi, pj, ni, nj;
    DevBuf<double> wts, dpos, dneg;
    DevBuf<i32> aidx;     // the fused fit's prepared tally operands (k_auc_prepare)
    DevBuf<double> afac;
};

// The link model of cge_link_* (link_host.cpp): the geometric Chung-Lu model of ONE alpha over the resident embedding and graph,
// p(i, j) = f_out[i] f_in[j] max(0, 1 - dist(i, j) / hi)^alpha.  Fitted (cge_link_fit: the sweep's own iterate at a best alpha,
// copied aside while the sweep runs) or supplied (cge_link_set_model).  Dropped by whatever replaces the resident inputs.
struct LinkModel {
    bool valid = false;
    int directed = 0;
    int pow_form = 0;        // the power as the sweep's local score took it: 0 the library pow, 1 log_parts + exp2_parts (pow_parts.hpp)
    double alpha = 0.0, hi = 0.0;
    i64 n = 0, NT = 0;       // vertices; iterates of a fitted model (landmarks, or vertices in exact mode; 0: supplied)
    DevBuf<double> f;        // f_out[n], f_in[n] (two copies of one vector when undirected)
    DevBuf<double> T;        // T_out[NT], T_in[NT], original numbering
    DevBuf<double> ftile;    // max of f_in over every 128 candidates (the top-k filter's bound), ldn / 128 entries
    // the resident edge list as sorted 64-bit keys (a << 32 | b; undirected: a <= b), built on the first top-k that excludes edges
    DevBuf<unsigned long long> keys, keys_in;
    i64 nkeys = 0;
    bool keys_ready = false;
    // per vertex the distinct excluded neighbours other than itself, derived from the keys on the first rank query that excludes edges
    DevBuf<i32> excl;
    bool excl_ready = false;
    DevBuf<double> fib;      // f_in[c]^(-1 / alpha), the candidate's part of the rank filter's root; built on the first rank query
    bool fib_ready = false;
    // cge_link_fit while its sweep runs: which best is wanted (0: no capture), and what was copied aside last
    int cap_which = 0;
    bool cap_have = false;
    double cap_alpha = 0.0, cap_hi = 0.0; // cap_hi: the diameter the sweep normalised by; cap_pow: the form of its power
    int cap_pow = 0;
    i64 cap_N = 0;
    DevBuf<double> cap_T;    // Ta[N], Tb[N] of the captured alpha, original numbering
    // scratch of the calls (grow-only)
    DevBuf<i32> ids;
    DevBuf<double> vals, Xq, rq, lp;
    DevBuf<i32> lj, lcnt;
    DevBuf<i64> oj, ocnt;
    DevBuf<unsigned long long> surv;
    i64 stat_survivors = 0, stat_queries = 0; // exact evaluations / queries of the last cge_link_topk
    // cge_link_rank: the distinct queries, their pairs grouped (offsets, thresholds descending, targets, the way back), the two
    // histograms, the results
    DevBuf<i32> ruq, rgj;
    DevBuf<i64> roff, rperm, rout;
    DevBuf<double> rt;
    DevBuf<unsigned long long> rhist;
    i64 stat_rank_survivors = 0, stat_rank_queries = 0; // exact evaluations / distinct queries of the last cge_link_rank
    // cge_link_sample: log2 of the factors (the filter's tables; built on the first draw), the edges' keys as appended and sorted,
    // the two counters, the ids on their way out
    DevBuf<double> lf;
    bool lf_ready = false;
    DevBuf<unsigned long long> skeys_in, skeys, scnt;
    DevBuf<i64> sout;
    i64 stat_sample_edges = 0, stat_sample_survivors = 0, stat_sample_tiles = 0; // of the last cge_link_sample
    // cge_link_auc: the positives' values sorted ascending and the way back to the edge list's order (the two histograms are
    // rhist, the counts in edge-list order rout, the values themselves vals), the counters
    DevBuf<double> at;
    DevBuf<i64> aperm;
    DevBuf<unsigned long long> acnt;
    i64 stat_auc_survivors = 0, stat_auc_tiles = 0, stat_auc_proven = 0; // of the last cge_link_auc
    // cge_link_moments: the centred operand, its norms and the factors in community order, the call's tables (i32 and i64), the
    // items' row / column partials and bin partials, the counters, the outputs (released with the model: link_drop)
    DevBuf<double> mXp, mrp, mf, mrow, mbin, mout;
    DevBuf<i32> mtab;
    DevBuf<i64> moff;
    DevBuf<unsigned long long> mcnt;
    i64 stat_mom_exact = 0, stat_mom_fast = 0, stat_mom_saturated = 0, stat_mom_tiles = 0; // of the last cge_link_moments
    // cge_link_triangles: the matrix Q (tld x tld, tld = k_link_tri_ld(n)), the tiles' row / column partials, the two outputs
    // (tri, wed), the counters (saturated pairs, long edges); the graph side's distinct degrees, triangle counts, oriented keys as
    // made and sorted, list offsets and long edges (released with the model: link_drop)
    DevBuf<double> tQ, tpart, tout;
    DevBuf<unsigned long long> tcnt, ttri, tokeys_in, tokeys;
    DevBuf<i32> tdeg;
    DevBuf<i64> toff, tlong;
    i64 stat_tri_tiles = 0, stat_tri_saturated = 0, stat_tri_bytes = 0; // of the last cge_link_triangles
};
// the tables of one cge_link_moments call on the device (link_host.cpp builds them, kernels_link.hip reads them)
struct LinkMomentsTables {
    const i32 *perm, *rank;       // position -> vertex; position -> rank of its community among those present
    const i32 *isi, *isj;         // the work items' blocks
    const i32 *bfr, *bnc;         // per block: first rank, ranks
    const i32 *cid, *rb0, *rb1;   // per rank: community (0-based), first and last block
    const i64 *boff;              // per item: first bin slot
    i64 wb, nT, nB, items, slots, Cp, C;
};

struct cge_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<hipEvent_t> event_pool; // recycled kernel-timer events
    PinBuf<unsigned char> stage[2];    // pinned staging of the uploads (cge_set_graph / cge_set_embedding)
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr; // device->host result copies that overlap the kernels queued behind them
    hipEvent_t copy_ev = nullptr, copy_done = nullptr;
    std::string err;
    int n_threads = 8;
    ThreadPool *pool = nullptr; // persistent host workers (n_threads - 1 + caller)
    cge_collectives coll{};
    cge_collectives_ext coll_ext{}; // optional further ops of the hook (all-gather, reduce-scatter)
    bool has_coll = false;
    int opt_wedges_rs = 0; // 1: the N x N landmark-pair matrix goes out by row blocks (reduce-scatter); 0 (default): all-reduce
    void *rccl_comm = nullptr;           // in-library communicator (collectives.cpp); takes precedence over the hook
    i64 stat_coll_calls = 0, stat_coll_bytes = 0; // all-reduces issued since the context was created
    DevBuf<double> xown;  // library-owned exchange buffer (cge_exchange_buffer)
    double *xptr = nullptr; // exchange buffer in use (library- or caller-owned)
    size_t xcap = 0;

    // ---- resident original graph --------------------------------------------------------
    i64 n = 0, m = 0, d = 0;   // m = edges RESIDENT on this rank (all of them unless the list is sharded, below)
    // N > 1 with option "shard_ingest": a rank uploads and keeps rows [e_first, e_first + m) of the caller's edge list only
    // (m_total = the caller's count); the embedding is uploaded as a slice of rows per rank and all-gathered over xGMI
    i64 m_total = 0, e_first = 0;
    bool edges_sharded = false;
    int opt_shard_ingest = 0;
    DevBuf<double> samp_xchg;  // sampled edges of a sharded list on their way through the all-reduce
    // N > 1 with option "shard_rows": the EMBEDDING ROWS are sharded BY COMMUNITY (north star: "edge list and embedding rows
    // shard across the GPUs").  A community lives on one rank (largest first, each to the least loaded rank); rank r keeps
    // the rows of its communities only: Xr is n_loc x d, local row i = the i-th owned vertex in ascending vertex id
    // (loc2glob / glob2loc, -1 = another rank's).  Everything that walks rows (runsplit, aggregation, the bound pass and the
    // sweeps of the diameter, row hashes) runs over LOCAL ids against Xr / vw_loc / comm_loc; the small per-vertex tables
    // (vw, comm, v2l: 4-8 bytes per vertex) stay replicated, global ids.  What crosses ranks is listed in DESIGN.md section 6.
    int opt_shard_rows = 0;
    bool rows_sharded = false;
    i64 n_loc = 0;
    std::vector<i32> h_loc2glob, h_glob2loc;
    std::vector<int> comm_owner;     // owner rank of community q (0-based)
    DevBuf<i32> loc2glob, glob2loc, comm_loc;
    DevBuf<double> vw_loc;
    std::vector<double> h_vw_loc;
    std::vector<i32> h_gl_off;       // landmark -> GLOBAL member counts as a prefix (N + 1); h_mem_off holds the LOCAL ones
    std::vector<int> lm_owner;       // owner rank of every landmark of the last run
    DevBuf<i32> v2l_loc;             // landmark of every local row
    bool wedges_block_only = false;  // the N x N landmark-pair matrix was reduce-scattered: only this rank's row block is summed
    bool unit_weights = false;
    bool blocked_ready = false; // blocked copy of the edge list (edge pass) matches src/dst
    DevBuf<i32> src, dst;     // 0-based
    DevBuf<double> w;         // edge weights
    DevBuf<double> Xr;        // n x d row-major (node-major)
    DevBuf<double> Xc;        // dpad x ldn feature-major, zero padded, centred at the global mean (diameter kernel)
    DevBuf<double> rnorm;     // ldn: squared norm of the centred rows (0 in the padding)
    i64 ldn = 0, dpad = 0;
    bool centred_ready = false;
    DevBuf<i32> comm;         // n, 0-based
    DevBuf<unsigned short> comm16; // the same as uint16 when C < 65536 (2 MB at n = 10^6: L2-resident gather table)
    DevBuf<double> vw;        // n
    // blocked copy of the edge list for the cluster-pair scatter (kernels_scatter.hip)
    DevBuf<unsigned> be_edge;           // m words (u mod 32768) << 16 | (v mod 32768), grouped by (block of u, block of v)
    DevBuf<double> be_w, be_wkeys, be_diag; // weights in that order (weighted lists); pass-1 outputs
    DevBuf<i32> be_chunk;               // be_nchunks x {block of u, block of v, first edge, edges}
    i64 be_nchunks = 0;
    i64 stat_layout_build_us = 0;       // wall time of the last build of the blocked copy (one-off per resident graph)
    int be_per = 16;                    // edges per thread of the edge pass the chunks were cut for (kernels_scatter.hip)
    DevBuf<unsigned short> be_keys, be_runoff;
    DevBuf<unsigned short> v2l16;       // uint16 landmark of every vertex (padded like comm16): table of the landmark-pair passes
    std::vector<double> h_Xr; // host mirror, row-major (cut rules + RSS run on the host)
    std::vector<i32> h_comm;
    std::vector<double> h_vw;
    std::vector<double> h_w;       // edge weights mirror (sample weights)
    i64 n_comm_max = 0;            // C of the original graph

    // ---- landmark state (output of cge_landmarks_run) ------------------------------------
    bool lm_ready = false;
    int lm_directed = 0;
    i64 N = 0;
    int lm_truncated = 0;
    std::vector<i64> h_v2l;   // 1-based landmark of each vertex
    std::vector<i32> h_v2l0;  // the same, 0-based (upload staging)
    DevBuf<i32> v2l;          // 0-based
    DevBuf<double> lemb;      // N x d row-major
    DevBuf<double> lweight, dii;
    DevBuf<i32> lcomm;        // 0-based
    DevBuf<double> wedges;    // N x N, [a*N + b]
    DevBuf<double> vectC;     // from the original edges
    i64 n_ledges = 0;
    bool wedges_ready = false; // the N x N landmark-pair matrix is built lazily (cge_score does not need it)

    // ---- scratch for host-array wGCL ------------------------------------------------------
    DevBuf<double> s_emb, s_dist, s_vw, s_vectC, s_degin, s_degout;
    DevBuf<i32> s_comm;
    DevBuf<double> auc_part, js_part;
    DevBuf<unsigned> js_counter; // bins_js_kernel's arrival counter (monotonic: js_launches x CGE_PARTIAL_BLOCKS arrivals so far)
    unsigned js_launches = 0;
    // alpha-sweep scratch (grow-only: no hipMalloc/hipFree inside a scoring call after the first)
    DevBuf<double> sw_D, sw_GD, sw_T1, sw_T2, sw_S1, sw_S2, sw_rowbins, sw_vectB, sw_scal, sw_lohi, sw_fitstate, sw_mm;
    DevBuf<int> sw_flags;
    DevBuf<unsigned long long> sw_fring;
    // The packed form of an undirected exact sweep (wgcl_host.cpp): GD of the current alpha as its upper 64 x 64 tiles only
    // (cge_packed_index below), made from the embedding rows every alpha; no D, no logarithm, no row-major GD
    DevBuf<double> sw_PK;
    int opt_exact_packed = 0;           // 0 auto (where the resident matrices would be refused), 1 whenever the form applies
    // the same form for a directed exact sweep (the model's matrix is symmetric; only Tin / Tout are not): 0 never (refused beyond
    // the resident limit), 1 where the resident matrices would be refused, 2 wherever the form applies
    int opt_exact_packed_directed = 0;
    int opt_test_fit_dir_tiles = 0;     // testing: a resident directed launch-per-iteration fit goes by the tile pair (kernels_fitp.hip)
    double opt_test_resident_limit = 0; // testing: replaces the 200e9 bytes of the resident form's guard (0: the default)
    int opt_test_cus = 0;               // testing: the CU count device_cus(c) reports, 1 .. the device's own (0: the device's own)
    i64 stat_exact_packed = 0;          // the last sweep ran packed
    i64 stat_exact_matrix_bytes = 0;    // O(N^2) device bytes the last exact sweep required
    bool sweep_used_fp_P = false;       // the running sweep fitted an alpha by one launch pair per iteration (fp_P)
    // persistent Chung-Lu fit (kernels_fitp.hip): T double buffer, partial vectors, per-workgroup maxima, barrier words
    DevBuf<double> fp_T, fp_Tsave, fp_P, fp_fpart, fp_Td, fp_flow;
    DevBuf<double> ls_eigscr;            // wide eigen-solver: partial vectors of its tile sweeps (kernels_lm.hip)
    bool bvec_contig = false;            // the score graph of the running sweep has contiguous communities (relabelled)
    bool bvec_blocks = false;            // ... and vect_B is summed by tiles (kernels_fit.hip: bvec_tile_kernel + bvec_bins_kernel)
    int opt_bvec_blocks = 0;             // 1: relabel the score graph of a sweep by community (from 256 vertices on) and sum vect_B by
                                         // tiles (measured slower: profiles/r04_bvec_tiles_ab.txt); 0 (default): the row-bin form
                                         // (relabelled only beyond 8192 vertices)
    DevBuf<i32> sw_bt_fc, sw_bt_ns, sw_bt_base; // per 64-vertex block: first community, communities; per tile: base of its partials
    i64 flow_armed_words = 0;            // > 0: the persistent fit's hand-off slots (that many 4-byte words) are armed by the previous alpha's last launch
    DevBuf<double> sw_bt_part;
    DevBuf<i32> sw_bt_desc;             // per community-pair bin: the positions of (up to four of) its tile partials (k_bins_prepare)
    DevBuf<double> sw_fused_pw;          // ... and the two powers per sample its prologue writes for its epilogue
    DevBuf<char> sw_fused_epi;           // the fused chain's tables, one cge_fit_fused per sample set (wgcl_host.cpp)
    int opt_fit_fused = 1;               // 1 (default): landmark-mode sweeps let the rest of an alpha's chain ride on the fit's launch
    i64 stat_fit_fused = 0;              // alphas of the last sweep that did
    // cge_score_batch (batch_host.cpp): the launch groups' scalars, vect_B, JS partials and hand-off slots; per call: multi-problem
    // fit launches and the member-alphas they fitted
    DevBuf<double> batch_scal, batch_vectB, batch_jspart, batch_flow;
    PinBuf<double> batch_pin;
    i64 stat_fit_batched_launches = 0, stat_fit_batched_alphas = 0;
    DevBuf<i32> sw_rl_order, sw_rl_comm; // exact mode, N > 8192: the score graph relabelled by community (wgcl_host.cpp)
    DevBuf<double> sw_rl_emb, sw_rl_vec, sw_rl_T;
    DevBuf<int> fp_flags;
    PinBuf<double> pin_scal;    // the scalars of an alpha (AUC sums, divergences, the fit's verdict), two alphas in flight
    hipEvent_t sweep_ev[2] = {nullptr, nullptr};
    int opt_pow_exp2 = 1; // (1 - D)^alpha as exp2(alpha * log2(1 - D)) with the logarithm computed once per score
    i64 pow_logs_N = 0;   // log2(1 - D) of the current sweep is in sw_Lh / sw_Ll (0: not prepared)
    bool pow_logs_upper = false;
    i64 pow_logs_blocked_N = 0; // ... or, for the fused persistent fit only, tile-blocked (kernels_fit.hip: log_matrix_tiles_kernel)
    DevBuf<double> sw_Lh;
    DevBuf<float> sw_Ll;
    bool opt_exact_relabel = true; // exact mode, N > 8192: relabel the score graph by community (wgcl_host.cpp)
    int opt_shard_samples = 1; // N > 1: 1 = local-score tallies split over the ranks from 10^5 samples on (in-library RCCL), 2 = always, 0 = never
    int opt_shard_forced = 1; // N > 1: the forced per-community phase of runsplit is split over the ranks
    int opt_test_rss2_one_kernel = 0; // testing: rss2 by rss2_walk_kernel at every width (the comparator of the chain + merge form)
    int opt_test_eig_roles = 0; // testing: the roles of group_eig_kernel's waves (0 by SIMD placement, 1 identity, 2 reversed, 3 rotated by
                                // one); the results must not depend on it
    int opt_test_pcent_form = 0; // testing: the form of the bf16-split bound pass (0 by the number of reference points, 1 streaming,
                                 // 2 register-resident); the results must not depend on it
    i64 opt_test_louvain_wave_len = -2; // testing: Louvain levels >= 2 decide segments longer than this by a wave (-2: the default
                                        // length, -1: every vertex, 2^31 - 1: none); the results must not depend on it
    int opt_ecg_group = 0; // cge_ecg: members that run their rounds in lock-step (0: chosen from the free memory, g >= 1: at most g)
    i64 stat_ecg_groups = 0, stat_ecg_member_rounds = 0, stat_ecg_peel_rounds = 0, stat_ecg_levels = 0; // last cge_ecg
    int opt_test_bvec_plain = 0; // testing: vect_B without LDS staging / rows in flight (the forms of very large score graphs)
    int opt_fit_persistent = 0; // 0 auto (score graphs of >= 128 vertices that fit the register file), 1 never, 2 whenever it fits
    i64 opt_fit_max_iters = 2000000; // a Chung-Lu fit that has not met `diff <= delta` (src/divergence.jl:151,434) after this many
                                     // iterations raises CGE_E_ASSERT -- the reference's loop has no bound and would not return
    int opt_fit_test_timeout = 0; // testing: the persistent fit gives up at once, so the fallback path runs
    int opt_fit_test_delay = 0;   // testing: the tile waves of the data-as-signal fits nap this many times (~3 us each) before
                                  // their first load -- start skew, as under contention; results must not change
    i64 stat_lm_batches = 0, stat_lm_rows = 0, stat_lm_splits = 0; // last runsplit: device batches, their rows, groups split (those of one
                                                                   // or two rows, which need no device batch, included)
    i64 stat_lm_pops = 0, stat_lm_failed = 0, stat_lm_take_rounded = 0; // last runsplit: groups popped by the replay (both phases), splits
                                                                        // computed that failed (popped or not), rounds whose batch the
                                                                        // 512 rule of 64 < d <= 128 cut down
    int opt_test_lm_speculate = 0; // testing: which groups a round of advance_heaps splits: 0 as ever, 1 the global phase splits the top of
                                   // its heap alone, 2 every candidate above the threshold (no `take` cut), 3 as 0 and the forced phase's
                                   // local heaps speculate too; the landmark ids do not depend on it
    DevBuf<int> cut_ties;                                          // last runsplit: tasks of the cut rules with a row ON the cut (device counter)
    i64 stat_fit_persistent = 0; // alphas fitted by the persistent kernel in the last sweep
    i64 stat_fit_iters = 0;      // Chung-Lu iterations of the last sweep (all alphas)
    // A hand-off of a persistent fit timed out (e.g. another process holds CUs): the rest of THIS sweep runs one launch per
    // iteration.  Not latched for the life of the context: the next sweep tries the persistent form again, backing off
    // (1, 3, 7, ... sweeps skipped) while the time-outs repeat; stat "fit_persistent_fallbacks" counts them.
    bool fit_persistent_broken = false;
    i64 stat_fit_fallbacks = 0;
    int fit_fallback_streak = 0;
    i64 fit_skip_sweeps = 0;
    DevBuf<i32> sw_cm_off, sw_cm_mem, sw_cm_pos; // community -> members CSR of the score graph and its inverse
    DevBuf<double> sw_zeros, sw_zsum;
    // diameter scratch
    DevBuf<MaxRec> mp_recs;
    DevBuf<i64> mp_count;
    DevBuf<int2> nt_pairs, nt_tiles; // near-tied pairs of the arg-max (vertex ids) / the tiles searched for them
    DevBuf<i32> nt_idx;              // the pairs' split index arrays
    DevBuf<double> nt_out, nt_rows; // their dist() values / the gathered rows (option shard_rows)
    DevBuf<double> mp_rd2, mp_refmu; // reference-point distances / centroids of the pruned diameter
    DevBuf<double> mp_commax;        // per-community maxima of the bound matrix (two-level candidate selection)
    DevBuf<int2> mp_plist;           // surviving community pairs
    DevBuf<i32> mp_lref, mp_refoff, mp_refmem;
    DevBuf<double> gmean;    // global feature mean (the centre used by Xc)
    bool emb_nonfinite = false; // a NaN / Inf in the resident embedding (seen in gmean): the diameter is NaN
    DevBuf<double> Xs, rns, Ms, mnorm, Pm; // landmark-sorted centred copy, centroids, P matrix
    DevBuf<double> pc_groups;              // per (16-row group, reference point) maxima of the bound pass
    DevBuf<float> Xs32, Ms32;              // fp32 copies: operands of the fp32-MFMA bound pass (upper bounds only)
    DevBuf<unsigned short> Xb16, Mb16;     // two-plane bf16 operands of the bf16-split bound pass
    DevBuf<int> dm_flag;                   // raised by the bf16 gather when a value is unfit for the split
    // exact stage of the pruned diameter: the candidate landmarks' rows gathered per round (centred, feature-major), their
    // norms, source rows and global vertex ids; the seed row of the farthest-point sweep (option shard_rows)
    DevBuf<double> xe, xe_rns, dm_seed;
    DevBuf<i32> xe_pos, xe_glob, xe_sub, dm_soffE;
    int opt_diameter_f32 = 2;              // the point-to-reference maxima: 2 = bf16 matrix pipe, operands split in two terms (K <= 128; else 1),
                                           // 1 = fp32-input MFMA, 0 = fp64 MFMA; 1 and 2 are upper bounds with a rigorous error margin
    DevBuf<i32> pos2node, sub_land, dm_soff, dm_memoff, dm_mem;
    DevBuf<BoundRec> bound_list;           // candidate landmark pairs
    DevBuf<int2> tile_list;                // a round's tiles (first row, first column)
    std::vector<i32> h_mem_off, h_mem;     // landmark -> members (ascending vertex id), host copy
    DevBuf<uint64_t> uniq_hash;            // row hashes of the unique-row check
    DevBuf<unsigned long long> uniq_table; // ... and the device set that counts the distinct ones
    int opt_diameter = 0;                  // 0 auto (pruned with brute-force fallback), 1 brute force, 2 pruned only
    i64 stat_cand_pairs = 0, stat_cand_tiles = 0; // last pruned run
    int stat_diameter_path = 0;            // 1 brute, 2 pruned
    double stat_last_hi = 0.0;
    i64 stat_hi_i = -1, stat_hi_j = -1; // its arg-max pair (0-based vertex ids)
    int stat_bound_pass = 0;            // bound pass of the last pruned diameter: 2 bf16-split, 1 fp32 MFMA, 0 fp64 MFMA
    i64 stat_nref = 0; // reference points of the last pruned diameter (communities or landmarks)
    // scratch of the batched split engine (landmarks_host.cpp)
    DevBuf<i32> ls_rows, ls_row_task, ls_ct, ls_cb, ls_ce, ls_co, ls_tco; // ls_co: the chunks' launch order (batch_tables)
    DevBuf<double> ls_part, ls_mean, ls_sw, ls_cov, ls_vec, ls_z, ls_sums;
    DevBuf<unsigned char> ls_side, ls_state;
    DevBuf<double> ls_params; // per-task round parameters of the rss rule
    PinBuf<double> pin_sums, pin_params;
    PinBuf<i32> pin_clusters;               // runsplit: the initial clusters on their way into the member arena
    PinBuf<i32> pin_hb_rows, pin_hb_row_task; // rows / row -> task of a host-built batch (the generic rss path)
    // sorted-prefix rss path
    DevBuf<i32> sp_srows, sp_meta, sp_rounds, sp_tro, sp_perm, sp_status, sort_idx, sort_idx2, sort_keys32, sort_k32b, sort_cnt;
    DevBuf<unsigned char> sort_keys8;
    // member lists of the landmark phase: a group is a range of this arena (vertex ids, reference order)
    DevBuf<i32> lm_arena;
    i64 lm_arena_used = 0;
    DevBuf<double> lm_means; // weighted means of groups, known from their parents' splits (d doubles each)
    i64 lm_means_used = 0;
    DevBuf<i64> ls_moff; // the groups' offsets into lm_means, one per task of a batch
    // small host <-> device tables of a landmark batch travel packed: one pinned staging area, one copy, one kernel that
    // scatters (gathers) the 4-byte words to (from) their device arrays (landmarks_host.cpp: WordPacker)
    PinBuf<i32> pin_tab[2], pin_res;
    DevBuf<i32> dev_tab, dev_res;
    hipEvent_t tab_ev[2] = {nullptr, nullptr};
    int tab_slot = 0;
    bool lm_index_on_device = false; // lm_memoff / lm_mem mirror h_mem_off / h_mem (set by runsplit, cleared when the host rebuilds the index)
    DevBuf<i32> ls_toff, ls_nlow, lm_goff, lm_glen, lm_mem, lm_memoff; // task arena offsets, low-child counts, final groups, landmark index
    DevBuf<unsigned char> ls_keys;
    PinBuf<i32> pin_small;
    DevBuf<unsigned char> sort_tmp;
    DevBuf<unsigned long long> sort_k64; // sorted 4096-row pieces of the long groups on their way to the rank merge

    DevBuf<double> sp_zs, sp_ctot, sp_coff, sp_prefix, sp_vals;
    DevBuf<double> r2_F, r2_ck;
    i64 r2_rows = 0;            // rows of the batch the rss2 kernels are about to see

    int opt_landmark_edges = 0;  // 1: cge_score builds the N x N landmark-pair matrix too (what landmarks() returns)
    // grow-only scratch of per-score helpers (no hipMalloc / hipFree inside a scoring call after the first: a hipFree waits
    // for every stream of the device)
    DevBuf<i32> epd_i, s_star;
    DevBuf<i64> wed_cnt;
    DevBuf<double> cc_dense; // dense C x C stage of vect_C beyond 2048 communities (tiled two-pass form)
    DevBuf<unsigned> samp_attempt;
    DevBuf<i32> samp_todo_a, samp_todo_b, samp_hit, samp_flag;
    DevBuf<unsigned long long> samp_table, samp_count;
    // a draw of the device sampler whose first round has been enqueued but not looked at yet (k_draw_samples_begin / _finish)
    struct DrawPending {
        bool on = false;
        i64 seed = 0, stream_id = 0, S = 0, cnt = 0;
        int directed = 0, round = 0;
        i32 *d_pos = nullptr, *d_ni = nullptr, *d_nj = nullptr;
        const i32 *todo = nullptr;
        i32 *next = nullptr;
    } samp_pending;
    PinBuf<unsigned long long> samp_pin_cnt;
    hipEvent_t samp_ev = nullptr;
    SampleSet smp;                 // library-drawn samples of the running score
    std::vector<std::unique_ptr<DevSamples>> dsets; // their device form (wgcl_host.cpp)

    LinkModel link;                // cge_link_* (link_host.cpp)

    // ---- profiling -------------------------------------------------------------------------
    bool profiling = false;
    std::vector<std::string> profile_only; // empty: every timer
    std::map<std::string, KernelTimer> timers;
    Phase phases;
};

// Bracket a launch with events when profiling is on.
struct ScopedKernelTimer {
    cge_ctx *c;
    KernelTimer *t = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedKernelTimer(cge_ctx *ctx, const char *name) : c(ctx) {
        if (!c->profiling) return;
        if (!c->profile_only.empty()) {
            bool hit = false;
            for (const std::string &n : c->profile_only) hit = hit || n == name;
            if (!hit) return;
        }
        t = &c->timers[name];
        a = take_event();
        b = take_event();
        (void)hipEventRecord(a, c->stream);
    }
    hipEvent_t take_event() { // events are recycled by flush_timers: no create/destroy in the timed region
        if (!c->event_pool.empty()) {
            hipEvent_t e = c->event_pool.back();
            c->event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    ~ScopedKernelTimer() {
        if (!t) return;
        (void)hipEventRecord(b, c->stream);
        t->pending.push_back({a, b});
        t->launches++;
    }
};

void flush_timers(cge_ctx *c); // capi.cpp: the event pairs of the finished launches become milliseconds, the events go back to the pool

#define CGE_FIT_TIMEOUT_TICKS 100000000LL // 1 s of the 100 MHz wall clock, re-armed at every Chung-Lu iteration
static inline void note_fit_fallback(cge_ctx *c) {
    if (c->opt_fit_test_timeout) return; // the testing hook abandons on purpose
    c->fit_persistent_broken = true;
    if (c->stat_fit_fallbacks++ == 0)
        fprintf(stderr, "libcge_hip: a persistent Chung-Lu fit timed out waiting for another workgroup (is the GPU shared?); "
                        "falling back to one launch per iteration for this sweep (stat fit_persistent_fallbacks)\n");
    c->fit_fallback_streak = std::min(c->fit_fallback_streak + 1, 6);
    c->fit_skip_sweeps = (1LL << (c->fit_fallback_streak - 1)) - 1;
}
// called at the start of a sweep: decide whether the persistent form is tried again
static inline void fit_sweep_begin(cge_ctx *c) {
    if (!c->fit_persistent_broken) return;
    if (c->fit_skip_sweeps > 0) { c->fit_skip_sweeps--; return; }
    c->fit_persistent_broken = false;
}

// the row space the landmark phase works in: all vertices, or this rank's rows (option shard_rows)
static inline i64 lm_rows(const cge_ctx *c) { return c->rows_sharded ? c->n_loc : c->n; }
static inline const double *lm_vw(const cge_ctx *c) { return c->rows_sharded ? c->vw_loc.p : c->vw.p; }
static inline const i32 *lm_comm(const cge_ctx *c) { return c->rows_sharded ? c->comm_loc.p : c->comm.p; }
static inline const double *lm_hvw(const cge_ctx *c) { return c->rows_sharded ? c->h_vw_loc.data() : c->h_vw.data(); }

static inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static inline i64 packed_len(i64 n) { return n * (n + 1) / 2; }
// 0-based packed upper-triangular index, i <= j  (== idx(n,i+1,j+1) - 1, src/auxilary.jl:57-59)
static inline i64 pidx0(i64 n, i64 i, i64 j) { return n * i - i * (i - 1) / 2 + (j - i); }

static inline unsigned grid_for(i64 work, int block, i64 cap = 256 * 8) {
    i64 g = (work + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

#define CGE_STAGE_BYTES ((size_t)64 << 20) // one staging buffer of the uploads (profiles/r05_microbench_upload.txt: 64 MiB chunks reach the link's 54-57 GB/s)
// Pageable host memory -> device through two pinned staging buffers: the host workers convert / copy chunk k into one
// buffer while chunk k-1 is on the wire from the other (a plain hipMemcpy from pageable memory is a single-threaded
// bounce copy).  fill(dst, e0, e1) writes elements [e0, e1) of the output into `dst` (e1 - e0 <= chunk) and may be
// called from several threads on disjoint sub-ranges.
template <typename T, typename F, typename A>
static void staged_upload_chunks(cge_ctx *c, T *dev, size_t total, size_t chunk, size_t dev_ring, F fill, A after) {
    for (int b = 0; b < 2; b++) c->stage[b].ensure(CGE_STAGE_BYTES);
    const int nt = std::max(1, std::min(c->n_threads, 8)); // (more fill threads than that slow the link down: profiles/r05_microbench_upload.txt)
    for (size_t off = 0, k = 0; off < total; off += chunk, k++) {
        const int b = (int)(k & 1);
        if (k >= 2) HIP_CHECK(hipEventSynchronize(c->stage_ev[b])); // the copy that last read this buffer is done
        const size_t len = std::min(chunk, total - off);
        T *dst = (T *)c->stage[b].p;
        const size_t per = (len + nt - 1) / nt;
        const std::function<void(i64)> job = [&](i64 t) {
            const size_t a = std::min(len, (size_t)t * per), e = std::min(len, a + per);
            if (e > a) fill(dst + a, off + a, off + e);
        };
        c->pool->run(nt, job);
        T *where = dev_ring ? dev + (k % dev_ring) * chunk : dev + off; // (a ring on the device: `after` consumes the chunk in stream order)
        HIP_CHECK(hipMemcpyAsync(where, dst, sizeof(T) * len, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipEventRecord(c->stage_ev[b], c->stream));
        after(where, off, len);
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
template <typename T, typename F>
static void staged_upload(cge_ctx *c, T *dev, size_t total, F fill) {
    // at least ~8 chunks, so that the fill of one overlaps the copy of the one before it (a 40 MB column of edge ids in one
    // 64 MiB chunk would be filled, then copied), of at least 2 MiB, at most a staging buffer
    const size_t cap = CGE_STAGE_BYTES / sizeof(T), lo = ((size_t)2 << 20) / sizeof(T);
    const size_t chunk = std::min(cap, std::max(lo, (total + 7) / 8));
    staged_upload_chunks<T>(c, dev, total, chunk, 0, fill, [](T *, size_t, size_t) {});
}

// ---- collectives.cpp: the exchanges between ranks, in place on the ctx stream (in-library RCCL, or the hook of
// cge_set_collectives through the exchange buffer); all of them do nothing without collectives ---------------------------------
void cge_allreduce_dev(cge_ctx *c, double *dev, i64 count, int op /*0 sum, 1 max of doubles, 2 sum of int64*/);
double cge_allreduce_scalar_max(cge_ctx *c, double v); // max of one double over the ranks (synchronises); v itself without collectives
void cge_allgather_dev(cge_ctx *c, double *buf, i64 words_per_rank); // world pieces of 8-byte words; this rank's piece is filled in
// sum of doubles over world blocks, rank r ends with block r.  true: went out by blocks; false: no such op here, the caller all-reduces
bool cge_reduce_scatter_dev(cge_ctx *c, double *buf, i64 words_per_rank);
// can the exchange buffer hold `need` doubles?  With the in-library communicator a library-owned buffer grows on demand
// (contents are not preserved); a caller-provided one (cge_set_exchange_buffer, the hook path) is what it is.
bool cge_exchange_fits(cge_ctx *c, size_t need);

// ---- graph_host.cpp: the resident graph and vertex data (what cge_set_graph / cge_set_vertex_data do; they throw) ---------------
// ONE ingest each: a cge_graph_view / cge_vertex_view (include/cge_hip.h); `who` names the entry point in messages.  set_graph /
// set_vertex_data are the views of their arguments (1-based int64 host columns, fp64 weights).
int graph_view_check(const cge_graph_view *g, i64 m, std::string &msg); // cge_graph_view_check; the message in `msg`
void set_graph_view(cge_ctx *c, const char *who, const cge_graph_view *g, i64 m, i64 n); // n = 0: the maximum id; c->n afterwards
// derive_vw: vweights == NULL means "derive them from the resident edge list" (else: leave the resident ones)
void set_vertex_view(cge_ctx *c, const char *who, const cge_vertex_view *v, i64 n, bool derive_vw);
void set_graph(cge_ctx *c, const int64_t *src, const int64_t *dst, const double *w, i64 m, i64 n);
void set_vertex_data(cge_ctx *c, const int64_t *comm, const double *vw, i64 n);
// clusters::Vector{Vector{Int}} of the resident communities (src/auxilary.jl:199-208), flat + offsets, 1-based ids (n_clusters = -1)
void clusters_from_comm(const cge_ctx *c, std::vector<i64> &flat, std::vector<i64> &off);
// kernels_graph.hip: a device-resident graph view made into the resident tables (ids: CGE_ID_*, stride in elements)
void k_id_extrema(cge_ctx *c, const void *a, const void *b, i64 stride, int id_dtype, i64 count, i64 *d_minmax); // b may be NULL
void k_graph_ingest(cge_ctx *c, const void *src, const void *dst, i64 stride, int id_dtype, i64 base, i64 n, const void *w, int w_dtype,
                    i64 m, i32 *osrc, i32 *odst, double *ow, i64 *flags); // flags[0] lowest bad edge (m: none), flags[1] some weight != 1
void k_vertex_ingest(cge_ctx *c, const void *ids, int id_dtype, i64 base, i64 n, i32 *comm, unsigned short *comm16);
void k_vertex_weights_unit(cge_ctx *c, const i32 *src, const i32 *dst, i64 m, i64 n, double *vw);
void k_vertex_weights_ordered(cge_ctx *c, const i32 *src, const i32 *dst, const double *w, i64 m, i64 n, double *vw);
void check_resident(cge_ctx *c, const char *who); // graph, embedding and vertex data resident and sized for one vertex set

// ---- embedding_host.cpp: everything that makes an embedding resident ----------------------------------------------------------
void set_embedding_view(cge_ctx *c, const char *who, const cge_embedding_view *v, i64 n); // the ingest; `who` names the entry point in messages
void cge_ensure_host_embedding(cge_ctx *c); // fetch the host mirror of Xr on first demand
bool ingest_sharded(const cge_ctx *c);      // N > 1 with option "shard_ingest": a rank uploads its share of the edge list / the rows
void rows_unshard(cge_ctx *c);              // option "shard_rows": drop the ownership tables (the rows are whole again)
void rows_refresh_local_tables(cge_ctx *c); // ... and re-make this rank's copies of the per-vertex tables
int view_check(const cge_embedding_view *v, i64 n, std::string &msg); // cge_embedding_view_check; the message in `msg`
void check_device_pointer(const cge_ctx *c, const char *who, const void *p); // CGE_E_ARG unless p is memory of the context's GPU

// ---- kernels_*.hip entry points (host launchers) ---------------------------------------------
// kernels_ingest.hip: an embedding view (dtype = CGE_DTYPE_*, ld in elements) widened into row-major fp64
size_t cge_dtype_size(int dtype);
void k_ingest_rows(cge_ctx *c, const void *src, int dtype, i64 ld, i64 rows, i64 d, double *dst); // dst[i * d + k] = src[i * ld + k]
// rows [i0, i0 + rows) x columns [k0, k0 + cols) of the row-major Xrow (row pitch d) from the column-major piece src[k * ld + i]
void k_ingest_cols(cge_ctx *c, const void *src, int dtype, i64 ld, double *Xrow, i64 rows, i64 cols, i64 i0, i64 k0, i64 d);
// out[i][k] = X[idx[i]][k] of a row-major (X[g * ld + k]) or column-major (X[k * ld + g]) matrix; a negative index: a zero row
void k_ingest_gather(cge_ctx *c, const void *X, int dtype, i64 ld, i64 d, int row_major, const i32 *idx, i64 cnt, double *out);
// the fp64 forms of the last two for scratch matrices (packed, no kernel timer: they run inside the diameter search and the sampler)
void k_transpose_to_rowmajor(cge_ctx *c, const double *Xcol, double *Xrow, i64 n, i64 d);
void k_gather_rows_f64(cge_ctx *c, const double *X, i64 n, i64 d, int row_major, const i32 *idx, i64 cnt, double *out);
void k_row_hash(cge_ctx *c, const double *Xrow, uint64_t *hash, i64 n, i64 d);
i64 k_count_distinct(cge_ctx *c, const uint64_t *hash, i64 n); // distinct values among the hashes (device set; synchronises)
// landmark split primitives (batched over tasks; rows = concatenated 0-based vertex ids)
void k_group_mean(cge_ctx *c, const double *Xr, const double *vw, const i32 *rows, const i32 *chunk_task,
                  const i32 *chunk_beg, const i32 *chunk_end, i64 n_chunks, const i32 *task_chunk_off, i64 n_tasks,
                  i64 d, double *part, double *mean, double *sw);
void k_group_cov(cge_ctx *c, const double *Xr, const double *vw, const i32 *rows, const i32 *chunk_task,
                 const i32 *chunk_beg, const i32 *chunk_end, const i32 *chunk_order, i64 n_chunks, const i32 *task_chunk_off,
                 i64 n_tasks, i64 d, const double *mean, double *part, double *cov);
void k_group_side_sums(cge_ctx *c, const double *Xr, const double *vw, const i32 *rows, const unsigned char *side,
                       const i32 *chunk_beg, const i32 *chunk_end, i64 n_chunks, const i32 *task_chunk_off, i64 n_tasks,
                       i64 d, double *part, double *out);
void k_side_values_means(cge_ctx *c, const double *sums, i64 n_tasks, i64 d, double *vals, double *means);
void k_sorted_prefix(cge_ctx *c, const double *Xr, const double *vw, const i32 *srows, const i32 *chunk_beg,
                     const i32 *chunk_end, i64 n_chunks, const i32 *task_chunk_off, i64 n_tasks, i64 d, double *ctot,
                     double *coff, double *prefix);
void k_rss2_walk(cge_ctx *c, const double *Xr, const double *vw, const i32 *srows, const i32 *task_row_off, i64 n_tasks, i64 d,
                 i32 *meta, double *vals, double *cmeans);
void k_cut_sides(cge_ctx *c, const double *z, const double *zs, const i32 *task_row_off, i64 n_tasks, int use_median,
                 unsigned char *side, i32 *nlow_out = nullptr, // nlow_out: rows of the low side per task (replaces k_side_counts)
                 int *tie_tasks = nullptr);                     // tie_tasks: counts the tasks that held a row with z == cut
void k_rss_rounds(cge_ctx *c, const double *Xr, const double *vw, const i32 *srows, const double *zs,
                  const i32 *task_row_off, const i32 *task_chunk_off, const double *prefix, const double *coff,
                  i64 n_tasks, i64 d, i32 *meta, i32 *rounds, double *vals, double *cmeans /* [task][2][d] */);
#define CGE_RR_MAXROUNDS 63
#define CGE_CHUNK_ROWS 1024 // rows per chunk of a batch (build_batch); the rounds kernel uses r >> 10
#define CGE_PARTIAL_BLOCKS 64 // block partials of the JS / AUC reductions (summed in block order)
// The scalars of one alpha as the device leaves them and the host reads them from a pinned slot (host_wgcl_sweep, and per member
// host_batch_sweep): the AUC block tallies (two per block), the shared verdict right behind them (one all-reduce(sum) covers
// both; the slot after it only keeps RES_JS 16-byte aligned), the JS block sums of two modes, the fit's flags.  RES_LEN doubles
// are copied out; an alpha's scalars are RES_STRIDE doubles apart.
constexpr i64 RES_AUC = 0, RES_VERD = 2 * CGE_PARTIAL_BLOCKS, RES_JS = RES_VERD + 2, RES_FIT = RES_JS + 2 * CGE_PARTIAL_BLOCKS,
              RES_LEN = RES_FIT + 2, RES_STRIDE = RES_FIT + 16;
#define CGE_PREFIX_STRIDE 8 // the sorted-order WSSE prefix is stored every 8th row of a chunk (CGE_CHUNK_ROWS % 8 == 0)
void k_gather_means(cge_ctx *c, const double *arena, const i64 *off, i64 T, i64 d, double *mean);
void k_gather_rows(cge_ctx *c, const i32 *arena, const i32 *task_off, const i32 *task_row_off, const i32 *chunk_task,
                   const i32 *chunk_beg, const i32 *chunk_end, i64 n_chunks, i32 *rows, i32 *row_task);
void k_rss_child_keys(cge_ctx *c, const i32 *perm, const i32 *row_task, const i32 *task_row_off, const i32 *meta,
                      const i32 *rounds, i64 R, i64 T, unsigned char *keys, i32 *nlow);
void k_side_counts(cge_ctx *c, const unsigned char *side, const i32 *task_row_off, i64 T, i32 *nlow);
void k_sort_children(cge_ctx *c, const unsigned char *keys, const i32 *rows, const i32 *task_row_off, const i32 *chunk_beg,
                     const i32 *chunk_end, const i32 *task_chunk_off, i64 n_chunks, i64 R, i64 T, int key_bits, i32 *out);
i64 k_groups_to_index(cge_ctx *c, const i32 *arena, const i32 *goff, const i32 *glen, i64 N, i64 n, i32 *v2l, i32 *mem);
void k_segmented_sort_z(cge_ctx *c, const double *z, const i32 *rows, const i32 *row_task, const i32 *task_row_off,
                        i64 R, i64 T, double *zs, i32 *perm, i32 *srows, i32 *status, i64 max_len = 0 /* longest group, 0: unknown */);
void k_rss_side(cge_ctx *c, const double *z, const i32 *row_task, i64 n_rows, const double *params,
                unsigned char *state, unsigned char *side);
bool k_group_eig(cge_ctx *c, const double *cov, i64 n_tasks, i64 d, double *vec);
void k_group_project(cge_ctx *c, const double *Xr, const double *vw, const i32 *rows, const i32 *row_task, i64 n_rows,
                     i64 d, const double *mean, const double *vec, double *z);
// landmark aggregation (src/landmarks.jl:387-430) with CSR landmark -> members (ascending vertex id)
void k_landmark_aggregate(cge_ctx *c, const double *Xr, const double *vw, const i32 *comm, const i32 *mem_off,
                          const i32 *mem, i64 N, i64 d, double *lemb, double *lweight, double *dii, i32 *lcomm);
// per-edge scatter
bool k_edge_scatter_blocked_applies(const cge_ctx *c, i64 C);
bool k_blocked_edges_possible(const cge_ctx *c);
void k_pack_upper(cge_ctx *c, const double *dense, i64 C, double *packed);
bool k_build_blocked_edges(cge_ctx *c);
void k_edge_scatter_blocked(cge_ctx *c, i64 c0, i64 c1, i64 C, int directed, double *vectC);
// the tiled form's geometry for N landmarks: tiles of 1 << rshift rows, keys of rshift + colbits bits, the dynamic LDS of the two
// passes; host arithmetic only (elt = 4 bytes per cell for unit weights, 8 for a weighted list); false: the form declines
struct WedgeGeometry { int rshift, colbits; i64 ntile, ntpad; size_t lds1, lds2; };
bool k_wedge_geometry(i64 N, size_t elt, i64 nchunks, WedgeGeometry *g);
// the N x N landmark-pair matrix by the tiled two-pass form (kernels_scatter.hip); false: does not apply
bool k_wedge_scatter_blocked(cge_ctx *c, const i32 *v2l, i64 N, i64 c0, i64 c1, int directed, double *wedges, i64 *positive,
                             const char *timer = "edge_scatter_wedges");
#define CGE_COMM16_PAD 32768 // the uint16 community table is padded to a multiple of the edge pass's vertex block
void k_edge_scatter(cge_ctx *c, const i32 *src, const i32 *dst, const double *w, i64 e0, i64 e1, const i32 *v2l,
                    const i32 *comm, i64 N, i64 C, int directed, double *wedges, double *vectC);
void k_edge_degrees(cge_ctx *c, const i32 *src, const i32 *dst, const double *w, i64 m, double *deg_out,
                    double *deg_in, i32 *star);
void k_wedge_degrees(cge_ctx *c, const double *wedges, i64 N, double *deg_out, double *deg_in, i32 *star);
void k_compact_count(cge_ctx *c, const double *wedges, i64 N, int directed, i64 *count, i64 row0 = 0, i64 row1 = -1);
void k_wedge_degrees_block(cge_ctx *c, const double *wedges, i64 N, i64 row0, i64 row1, double *out3N);
void k_degrees_unpack(cge_ctx *c, const double *in3N, i64 N, double *deg_out, double *deg_in, i32 *star);
void k_louvain_level1(cge_ctx *c, i64 *comm_out_host, i64 *n_comm, double *quality, i64 *rounds); // kernels_louvain.hip
// the whole hierarchy (or its first max_levels > 0 levels): returns their number, writes the first levels_cap of them
i64 k_louvain_levels(cge_ctx *c, i64 max_levels, i64 levels_cap, i64 *comm_out_host, i64 *n_comm, double *quality, i64 *rounds);
// ECG (kernels_louvain.hip): K relabelled level-1 members, the 2-core, the reweighted graph, the hierarchy on it.  The `member_*`
// and `core_out` host arrays are the testing hook's (all NULL otherwise); members_only stops after the peel
struct EcgHostOut {
    i64 *comm = nullptr, *n_comm = nullptr;
    double *q = nullptr, *q_ecg = nullptr, *edge_w = nullptr;
    i64 *member_comm = nullptr, *member_nc = nullptr, *member_rounds = nullptr;
    double *member_q = nullptr;
    i32 *core = nullptr;
};
void k_ecg(cge_ctx *c, i64 K, double w_min, i64 seed, i64 final_level, bool members_only, const EcgHostOut &o);
// distances
void k_dist_matrix(cge_ctx *c, const double *emb, const double *diag, i64 N, i64 d, double *D);
void k_minmax_upper(cge_ctx *c, const double *D, i64 N, double *lo_hi);
void k_normalise(cge_ctx *c, double *D, i64 N, const double *lo_hi);
// The packed form of an exact sweep (kernels_dist.hip): the extrema of D over j >= i without storing D, and GD of one alpha
// straight from the embedding rows into the upper tiles (cge_packed_index).  pow_method: 1 = exp2 of the logarithm, 0 = library pow
void k_packed_extrema(cge_ctx *c, const double *emb, const double *diag, i64 N, i64 d, double *lo_hi);
void k_packed_gd(cge_ctx *c, const double *emb, const double *diag, i64 N, i64 d, const double *lo_hi, double alpha,
                 int pow_method, double *PK);
void k_max_pair(cge_ctx *c, const double *Xc, const double *rnorm, i64 n, i64 ldn, i64 dpad, int part, int nparts,
                double *best_val, i64 *best_i, i64 *best_j, std::vector<double> *wg_best = nullptr);
void k_pair_dist(cge_ctx *c, const double *Xr, i64 d, const i32 *pi, const i32 *pj, i64 S, double inv_scale_den,
                 double *out);
void k_diameter_layout(cge_ctx *c, const i32 *mem_off, const i32 *mem, const i32 *soff, i64 N, i32 *pos2node, i32 *sub_land,
                       i64 n_sub);
void k_pcent(cge_ctx *c, const double *Xs, const double *rns, i64 lds_rows, const double *Ms, const double *mnorm,
             i64 ldm, i64 n_land, i64 N, i64 dpad, const i32 *soff, double *P, int part = 0, int nparts = 1);
void k_max_pair_tile_list(i64 ldn, int part, int nparts, const std::vector<double> &wg, double thr, std::vector<int2> &out);
i64 k_pair_collect(cge_ctx *c, const double *Xs, const double *rns, i64 ld, i64 nrows, i64 dpad, const int2 *tiles, i64 t0, i64 t1,
                   int tri, double thr, const i32 *ids, int2 *out, i64 cap);
void k_pair_list(cge_ctx *c, const double *Xs, const double *rns, i64 lds_rows, i64 npos, i64 dpad, const int2 *tiles,
                 i64 ntiles, double *best_val, i64 *best_i, i64 *best_j, std::vector<double> *wg_best = nullptr);
i64 k_bound_select(cge_ctx *c, const double *Q, const i32 *lref, i64 N, i64 nref, double L, BoundRec *list, i64 cap,
                   const i32 *ref_off = nullptr, const i32 *ref_mem = nullptr);
void k_ref_dist2_fm(cge_ctx *c, const double *Ms_fm, i64 nref, i64 dpad, i64 ldm);
i64 k_argmax_mapped(cge_ctx *c, const double *v, i64 n, const i32 *map, double *val = nullptr);
void k_pair_local_idx(cge_ctx *c, const i32 *pi, const i32 *pj, i64 S, const i32 *glob2loc, i32 *idx);
void k_pair_dist_rows(cge_ctx *c, const double *B, i64 d, const i32 *pi, const i32 *pj, i64 S, double den, double *out);
void k_position_ids(cge_ctx *c, const i32 *pos2node, const i32 *loc2glob, i64 npos, i32 *ids); // map[argmax v] (synchronises the stream)
void k_ref_centroids(cge_ctx *c, const double *mu, const double *lw, const i32 *ref_off, const i32 *ref_mem, i64 nref,
                     i64 d, double *out);
void k_farthest_enqueue(cge_ctx *c, const double *Xr, i64 n, i64 d, i64 src, const double *srow = nullptr); // launch only (c->stream) ...
void k_farthest_collect(cge_ctx *c, double *best_val, i64 *best_i);            // ... and its result (synchronises c->stream)
void k_col_mean(cge_ctx *c, const double *Xrow, i64 n, i64 d, double *mean, double sums_only = 0.0);
void k_scale_vector(cge_ctx *c, double *v, i64 n, double f);
void k_pack_landmarks(cge_ctx *c, double *lemb, double *lweight, double *dii, i32 *lcomm, i64 N, i64 d, double *X, int unpack);
void k_scatter_u64(cge_ctx *c, const uint64_t *src, const i32 *idx, i64 cnt, uint64_t *dst);
void k_scatter_i32(cge_ctx *c, const i32 *src, const i32 *idx, i64 cnt, i32 add, i32 *dst); // dst[idx[i]] = src[i] + add
void k_add_i32(cge_ctx *c, const i32 *src, i64 n, i32 add, i32 *dst);
void k_gather_centre_fm(cge_ctx *c, const double *src_rowmajor, const i32 *idx, const double *mean, double *dst,
                        double *rnorm, i64 npos, i64 d, i64 ld, i64 dpad, float *dst32 = nullptr,
                        unsigned short *planes = nullptr, i64 KP = 0, int *flag = nullptr); // planes: two bf16 terms, row-major [2][ld][KP]
void k_pcent_f32(cge_ctx *c, const float *Xs32, const double *rns, i64 lds_rows, const float *Ms32, const double *mnorm,
                 i64 ldm, i64 n_land, i64 N, i64 dpad, const i32 *sub_land, double *P, int part = 0, int nparts = 1);
// the bound pass on the bf16 matrix pipe with two-term operands (kernels_dist.hip (2c))
bool k_pcent_bf16_applies(i64 dpad);
void k_pcent_bf16(cge_ctx *c, const unsigned short *Xb, const double *rns, i64 lds_rows, const unsigned short *Mb,
                  const double *mnorm, i64 ldm, i64 n_land, i64 N, i64 KP, const i32 *sub_land, double *P, int part = 0, int nparts = 1);
// alpha sweep
void k_wave_tree_test(cge_ctx *c, const double *x, i64 n_rows, double *out_ref, double *out_new); // testing hook
void k_copy_segments(cge_ctx *c, const i32 *src, const i64 *seg, i64 nseg, i32 *dst);
void k_permute_rows(cge_ctx *c, const double *src, const i32 *order, i64 n, i64 width, double *dst); // dst[q] = src[order[q]]
void k_permute_i32(cge_ctx *c, const i32 *src, const i32 *order, i64 n, i32 *dst);
void k_remap_i32(cge_ctx *c, i32 *idx, const i32 *map, i64 n); // idx[k] = map[idx[k]]
#define CGE_WORD_SEGS 8
void k_copy_words(cge_ctx *c, int nseg, void *const *dst, const void *const *src, const i64 *words); // 4-byte words, nseg <= 8
// Several small host arrays -> their device arrays with ONE copy: the words are packed into a pinned staging buffer
// (two of them alternate, each guarded by an event), copied to a device staging area and scattered by one kernel.
// Every copy of its own from pageable memory costs ~20 us of idle stream; a batch has seven of them.
struct WordPacker { // (landmarks_host.cpp: the tables of a batch; wgcl_host.cpp: the tables of a sweep)
    cge_ctx *c;
    std::vector<void *> dst;
    std::vector<const void *> src;
    std::vector<i64> words;
    explicit WordPacker(cge_ctx *c_) : c(c_) {}
    template <class T>
    void add(T *device, const T *host, i64 count) {
        static_assert(sizeof(T) % 4 == 0, "4-byte words");
        if (count <= 0) return;
        dst.push_back(device);
        src.push_back(host);
        words.push_back(count * (i64)(sizeof(T) / 4));
    }
    void flush() {
        if (dst.empty()) return;
        i64 tot = 0;
        for (i64 w : words) tot += w + (w & 1); // keep 8-byte items aligned
        const int slot = c->tab_slot;
        c->tab_slot ^= 1;
        HIP_CHECK(hipEventSynchronize(c->tab_ev[slot])); // the copy that last read this staging buffer is done
        c->pin_tab[slot].ensure((size_t)tot);
        c->dev_tab.ensure((size_t)tot);
        i32 *h = c->pin_tab[slot].p;
        std::vector<const void *> dsrc(dst.size());
        i64 pos = 0;
        for (size_t q = 0; q < dst.size(); q++) {
            std::memcpy(h + pos, src[q], (size_t)words[q] * 4);
            dsrc[q] = c->dev_tab.p + pos;
            pos += words[q] + (words[q] & 1);
        }
        HIP_CHECK(hipMemcpyAsync(c->dev_tab.p, h, sizeof(i32) * (size_t)tot, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipEventRecord(c->tab_ev[slot], c->stream));
        for (size_t q0 = 0; q0 < dst.size(); q0 += CGE_WORD_SEGS) {
            const int n = (int)std::min<size_t>(CGE_WORD_SEGS, dst.size() - q0);
            k_copy_words(c, n, &dst[q0], &dsrc[q0], &words[q0]);
        }
        dst.clear(); src.clear(); words.clear();
    }
};
void k_gather_means_slots(cge_ctx *c, const double *arena, const i64 *off, const i64 *slot, i64 T, i64 d, i64 stride, i64 lead,
                          double *dst);
void k_pow_prepare(cge_ctx *c, const double *D, i64 N, bool upper_only, bool blocked = false);
void k_pow_matrix(cge_ctx *c, const double *D, i64 N, double alpha, double *GD, bool upper_only = false);
void k_pow_matrix_from(cge_ctx *c, const double *D, const double *Lh, const float *Ll, i64 N, double alpha, double *GD,
                       bool upper_only = false); // the same kernels on a caller's logarithm (Lh == nullptr: the library pow on D)
void k_pow_test(cge_ctx *c, const double *x, i64 n, double alpha, int method, double *out);
// What rides on the launch of the undirected persistent fit in a landmark-mode sweep relabelled by community (round 5): the
// power matrix computed in the prologue from the stored logarithm, vect_B's tile partials and the local score's tallies in the
// epilogue (kernels_fitp.hip: fit_flow_kernel<.., true>).  partial / auc_part == nullptr in the host copy: that part is not
// wanted this alpha (the device copy, written once per sweep and sample set, always holds both).
#define CGE_FLOW_NP 32 // runs of one community inside an 8-column chunk ("pieces") per 64-vertex block at most
struct cge_fit_fused {
    const double *Lh; const float *Ll; double alpha;   // host copy only: log2(1 - D) in two parts, this alpha
    const i32 *comm, *fc, *ns, *base; double *partial; // vect_B by tiles (relabelled sweep: communities are ranges of vertices)
    // the local score's samples, prepared once per sweep and sample set (k_auc_prepare): everything that depends neither on
    // alpha nor on T -- T's indices in the sweep's numbering [4][S], the factors vw_i, lw_li, vw_j, lw_lj, ... [8][S], the
    // weight sums of the CGE_PARTIAL_BLOCKS blocks -- and per alpha the two powers [2][S], which the fit's prologue writes
    i64 S; const double *dpos, *dneg, *wts; const i32 *aidx; const double *afac, *aden; double *apw; double *auc_part;
};
bool k_fit_flow_enqueue(cge_ctx *c, const double *GD, i64 N, const double *T0, double *Tout, i64 Tld, const double *w,
                        double eps, double delta, int *dev_flags, const cge_fit_fused *ff = nullptr,
                        const cge_fit_fused *ff_dev = nullptr); // ff_dev: the device copy of *ff the epilogue reads (alpha, partial and
                                                                // auc_part are taken from *ff: they change per alpha)
// The ONE launch geometry of the persistent fits, undirected and directed, single and shared (kernels_fitp.hip): Nt x Nt blocks
// of 64, NT upper tiles, G workgroups of NW waves (4 or 8), NSB = quarter blocks a workgroup may have to reduce (1 or 2).
struct FlowGeometry {
    int Nt; i64 NT; int G, NW, NSB;
    bool fused() const { return NSB == 1; } // what the fused and the shared instances exist for: one quarter block per workgroup
};
// the CU count of the current device as this context's launch shapes see it: the testing knob test_device_cus, which only shrinks
// it, else (and with `own`) the device's own
int device_cus(const cge_ctx *c, bool own = false);
bool flow_geometry(i64 N, int cus, FlowGeometry *g); // no device needed; false (g untouched): the persistent form does not apply
bool flow_geometry(const cge_ctx *c, i64 N, FlowGeometry *g); // on device_cus(c)
inline bool flow_fused_applies(const cge_ctx *c, i64 N) { FlowGeometry g; return flow_geometry(c, N, &g) && g.fused(); }
// whether cge_score_batch shares the fit of a member of N landmarks: N >= 256 and fused; directed also G <= cus / 2
bool flow_batch_member(i64 N, int cus, bool directed, FlowGeometry *g);
// The ONE layout of a problem's hand-off slots, as offsets in doubles from the region's start: 32 doubles of sync words, the T ring
// (4 Tld, directed 8 Tld), f (12 Nt), P (2 Nt^2 64, directed 4 Nt^2 64); `doubles` = the region (even: armed in 16-byte units)
struct FlowSlots { i64 sync, ring, fq, P, doubles; };
FlowSlots flow_slots(int Nt, i64 Tld, bool directed);
void k_bins_prepare(cge_ctx *c, const i32 *cm_off, i64 N, i64 C, i64 n_partials); // once per sweep, behind the tile tables
// what bins_js_kernel, the last launch of an alpha's chain, does on the way out: the alpha's scalars straight into the host's
// pinned slot (host_out; scal = their device copy, [res_js, res_js + 2 x CGE_PARTIAL_BLOCKS) = the JS partials this launch
// computes), and the sentinel fill of the next alpha's persistent fit (arm: 16-byte units)
struct cge_chain_tail {
    double *host_out; const double *scal; int res_js, res_len;
    uint4 *arm; i64 arm_n16; unsigned arm_word;
};
void k_bins_js(cge_ctx *c, const i32 *cm_off, i64 N, i64 C, const double *vC, double *vectB, int n_modes, double *fpart,
               const cge_chain_tail *tail = nullptr);
bool k_fit_flow_arm_region(cge_ctx *c, i64 N, i64 Tld, uint4 **ptr, i64 *n16, unsigned *word); // the fit's hand-off slots (for the tail above)
// ---- cge_score_batch: several fused fits in one launch, and the bins / JS launches of all of them (kernels_fitp.hip, kernels_fit.hip)
// One problem of fit_flow_multi_kernel: the arguments of its fit_flow_kernel<1, NW, true, 1> launch (and its FlowFused), its
// grid size G and its first workgroup wg0 in the concatenated grid
struct cge_flow_problem {
    const double *Lh; const float *Ll; double alpha; const cge_fit_fused *epi; int want, pad0;
    const double *T0; double *Tout; const double *w;
    double *ring, *P, *fq; unsigned *sync; int *flags;
    i64 N, Tld; int Nt, G, wg0, pad1;
};
// a problem's entry of the shared launch's table, as every caller fills it (the slots and wg0 are k_fit_flow_multi's); want: bit 0
// vect_B's tile partials, bit 1 the tallies of epi (0: nothing of the epilogue)
inline cge_flow_problem flow_problem_entry(const double *Lh, const float *Ll, double alpha, const cge_fit_fused *epi, int want,
                                           const double *T0, double *Tout, const double *w, int *flags, i64 N, i64 Tld,
                                           const FlowGeometry &g) {
    cge_flow_problem q{};
    q.Lh = Lh; q.Ll = Ll; q.alpha = alpha;
    q.epi = epi; q.want = want;
    q.T0 = T0; q.Tout = Tout; q.w = w;
    q.flags = flags;
    q.N = N; q.Tld = Tld; q.Nt = g.Nt; q.G = g.G;
    return q;
}
#define CGE_BATCH_MAX 16 // problems per launch group (G >= 16 for every fused problem: 256 CUs hold no more than 16)
struct cge_flow_multi { cge_flow_problem p[CGE_BATCH_MAX]; int n, pad; }; // passed by value (kernel arguments)
// lay the problems' slots out in `flow` (flow_slots each, in order), arm them all and launch (timer "fit_batched"); ring / P / fq /
// sync and wg0 are filled in here.  The problems share NW.  CGE_E_ASSERT for more than CGE_BATCH_MAX problems or a sum of G
// above the CU count (the caller packs them).
void k_fit_flow_multi(cge_ctx *c, cge_flow_multi &tab, int NW, double eps, double delta, DevBuf<double> &flow);
bool k_fit_flow_multi_fits(int NW, bool directed); // fit_flow_multi_kernel / fit_flow_dir_multi_kernel of NW waves gets a workgroup on a CU
// The same for directed graphs.  One problem of fit_flow_dir_multi_kernel: the arguments of its fit_flow_dir_kernel<NW, 1> launch
// (Tin / Tout: N doubles each, updated in place on success only), its grid size G and its first workgroup wg0.
struct cge_flow_dir_problem {
    const double *GD, *T0; double *Tin, *Tout; const double *deg_in, *deg_out;
    double *ring, *P, *fq; unsigned *sync; int *flags;
    i64 N, Tld; int Nt, G, wg0, pad;
};
struct cge_flow_dir_multi { cge_flow_dir_problem p[CGE_BATCH_MAX]; int n, pad; }; // passed by value (kernel arguments)
// the same, with T_0 = (Tin, Tout) zero-padded to Tld staged behind the slots (T0 is filled in here too); eps0, f0, delta are
// common to the launch
void k_fit_flow_dir_multi(cge_ctx *c, cge_flow_dir_multi &tab, int NW, double eps0, double f0, double delta, DevBuf<double> &flow);
struct cge_bins_problem { const double *partial; const i32 *cm_off, *fc, *ns, *base; i64 C; int Nt, pad; double *vectB; };
struct cge_js_problem { const double *vC, *vB; i64 len, C; int mode, pad; double *part, *fpart; };
struct cge_bins_multi { cge_bins_problem p[CGE_BATCH_MAX]; };
struct cge_js_multi { cge_js_problem p[2 * CGE_BATCH_MAX]; }; // (--split-global: two entries per problem)
void k_bins_js_multi(cge_ctx *c, const cge_bins_multi &bins, int n_bins, i64 max_C, const cge_js_multi &js, int n_js);
void k_bvec_tiles(cge_ctx *c, const double *GD, const double *Ta, const double *Tb, const i32 *cm_off, i64 N, int directed,
                  bool packed = false); // the tile partials only (packed: GD is the upper tiles of cge_packed_index)
void k_auc_prepare(cge_ctx *c, const i32 *v2l, const i32 *old2new, const double *vw_orig, const double *lweight, const i32 *pi,
                   const i32 *pj, const i32 *ni, const i32 *nj, const double *wts, i64 S, i32 *aidx, double *afac, double *aden);
void k_bvec_bins(cge_ctx *c, const i32 *cm_off, i64 N, i64 C, int directed, double *vectB); // folds the tile partials into vect_B
bool k_fit_persistent_dir(cge_ctx *c, const double *GD, i64 N, double *Tin, double *Tout, const double *deg_in,
                          const double *deg_out, double eps0, double f0, double delta, i64 *iters, int *dev_flags = nullptr,
                          bool *enqueued_only = nullptr);
void k_fit_verdict(cge_ctx *c, const int *flags, int async, double *out); // 1.0 when an enqueued fit was abandoned
// the same iteration over the upper 64 x 64 tiles only (kernels_fitp.hip): half the matrix traffic
void k_fit_sym_step(cge_ctx *c, const double *GD, const double *Tin, double *Tout, const double *w, i64 N, double eps,
                double delta, int k, unsigned long long *fring, int *done, int *iters, bool packed = false);
void k_fit_sym_dir_step(cge_ctx *c, const double *GD, const double *Tin, const double *Tout, double *Tin_n, double *Tout_n,
                        const double *deg_in, const double *deg_out, i64 N, double eps0, double f0, double delta, int k,
                        unsigned long long *fring, double *ering, int *done, int *iters, bool packed);
void k_fit_symv_dir(cge_ctx *c, const double *GD, const double *Tin, const double *Tout, i64 N, double *Sin,
                    double *Sout, const int *done);
void k_fit_update_dir(cge_ctx *c, double *Tin, double *Tout, const double *Sin, const double *Sout,
                      const double *deg_in, const double *deg_out, i64 N, double delta, int *done, int *iters,
                      double *state /* [0]=eps,[1]=diff */);
void k_bvec(cge_ctx *c, const double *GD, const double *Ta, const double *Tb, const i32 *cm_pos, const i32 *cm_off,
            const i32 *cm_mem, i64 N, i64 C, int directed, double *rowbins, double *vectB, int form = 0);
int k_bvec_form(const cge_ctx *c, i64 N); // the form k_bvec takes: 1 staged row bins, 2 plain gather, 3 contiguous rows, 4 tiles + bins
void k_js(cge_ctx *c, const double *vC, const double *vB, i64 len, i64 C, int directed, int mode /*0 all,1 int,2 ext*/,
          double *out, double *partials = nullptr);
void k_auc_landmark(cge_ctx *c, const double *Ta, const double *Tb, const i32 *v2l, const double *vw_orig,
                    const double *lweight, const i32 *pi, const i32 *pj, const i32 *ni, const i32 *nj,
                    const double *dpos, const double *dneg, const double *wts, i64 S, double alpha, double *out2, double *partials = nullptr);
void k_auc_exact(cge_ctx *c, const double *GD, const double *Ta, const double *Tb, i64 N, const i32 *pi,
                 const i32 *pj, const i32 *ni, const i32 *nj, const double *wts, i64 S, double *out2, double *partials = nullptr,
                 bool packed = false);
void k_gather_i32(cge_ctx *c, const i32 *arr, const i32 *idx, i64 S, i32 *out); // kernels_fit.hip: out[k] = arr[idx[k]]
void k_mark_edge_hits(cge_ctx *c, const i32 *src, const i32 *dst, i64 m, int directed, const uint64_t *table,
                      i64 table_size, i32 *hit);

// kernels_link.hip: the link model's kernels
// f_out[v] = (Ta[l] vw[v]) / lw[l], f_in[v] likewise from Tb, l = v2l[v] -- auc_landmark_kernel's own factors; v2l == nullptr: f = T
void k_link_expand(cge_ctx *c, const double *Ta, const double *Tb, const i32 *v2l, const double *vw, const double *lw, i64 n,
                   double *f_out, double *f_in);
void k_link_tile_max(cge_ctx *c, const double *f_in, i64 n, i64 ntiles, double *ftile); // max over every 128 entries
void k_link_prob(cge_ctx *c, const i32 *pi, const i32 *pj, i64 P, double *out);        // the resident model on 0-based pairs
void k_link_keys(cge_ctx *c);                                                           // the sorted edge keys of the model
// the top-k lists of Q queries (0-based ids, device) against every vertex: out_j (1-based) / out_p (Q x k), out_cnt (Q), device
void k_link_topk(cge_ctx *c, const i32 *qid, i64 Q, int k, bool exclude, i64 *out_j, double *out_p, i64 *out_cnt);
void k_link_excl(cge_ctx *c); // per vertex the distinct excluded neighbours, from the sorted keys (builds those when needed)
// a chunk of Qu distinct queries uq (off: their Qu + 1 offsets into the grouped thresholds t) counted into the histograms G / E
void k_link_rank(cge_ctx *c, const i32 *uq, const i64 *off, i64 Qu, const double *t, unsigned long long *G,
                 unsigned long long *E, bool exclude);
// the histograms of all Qu queries turned into greater / ties / cand, written through perm to the caller's order
void k_link_rank_final(cge_ctx *c, const i32 *uq, const i64 *off, i64 Qu, const double *t, const i32 *gj, const i64 *perm,
                       const unsigned long long *G, const unsigned long long *E, bool exclude, i64 *out_greater, i64 *out_ties,
                       i64 *out_cand);
// one draw of the model's random graph: the keys (a << 32 | b, 0-based) of the pairs with u < p appended to keys[cap] in no order,
// cnt[0] += their number (beyond cap: counted, not stored), cnt[1] += the pairs evaluated exactly; U != nullptr: the uniforms are
// read from that n x n matrix (the testing hook).  Returns the number of tiles walked
i64 k_link_sample(cge_ctx *c, i64 seed, i64 stream_id, unsigned long long *keys, i64 cap, unsigned long long *cnt, const double *U,
                  int ulay);
void k_link_auc(cge_ctx *c, int part, int nparts, const double *p, double *t, i64 *perm, unsigned long long *G, unsigned long long *E,
                unsigned long long *cnt, i64 *out_less, i64 *out_ties);
void k_link_sample_finish(cge_ctx *c, const unsigned long long *keys_in, unsigned long long *keys, i64 ne, i32 *pi, i32 *pj, i64 *oi,
                          i64 *oj);
i64 k_link_moments_wb(i64 nT); // tiles a block edge of cge_link_moments' work items, from the tile count alone
// the sums of the model over every pair (LinkModel's m* buffers sized by the caller): deg (n, directed 2 n), B and V (L each)
void k_link_moments(cge_ctx *c, const LinkMomentsTables &T, double *deg, double *B, double *V, i64 L, unsigned long long *cnt);
// kernels_linktri.hip: expected and observed triangles of the link model
i64 k_link_tri_ld(i64 n); // Q's leading dimension: n padded to an odd number of 128-tiles
void k_link_tri_q(cge_ctx *c, double *Q, i64 ld, unsigned long long *sat); // Q = min(p, 1), zero diagonal and padding; *sat = pairs p > 1
// tri[v] = rowsum(Q o (Q Q))[v] / 2 through the partials `part` (nT^2 128, nT = ceil(n / 128)), wed[v] = sum_{j<k} q_vj q_vk; either
// output may be nullptr (its kernels are not launched).  Returns the 128 x 128 tiles walked
i64 k_link_tri_expected(cge_ctx *c, const double *Q, i64 ld, double *part, double *tri, double *wed);
// the resident edge list as a simple undirected graph: deg (n) = distinct neighbours, tri (n) = triangles through the vertex
void k_link_tri_observed(cge_ctx *c, i32 *deg, unsigned long long *tri, unsigned long long *okeys_in, unsigned long long *okeys,
                         i64 *off, i64 *lng, unsigned long long *nlng);
// ---- host modules -----------------------------------------------------------------------------
// landmarks_host.cpp
void host_runsplit(cge_ctx *c, const i64 *cl_flat, const i64 *cl_off, i64 ncl, i64 nland, i64 forced, int method,
                   std::vector<i64> &group_ids /*0-based*/, bool want_index = false); // also fills c->v2l / lm_mem / lm_memoff (device)
void host_eig_top(const double *A, i64 d, double *v); // largest-eigenvalue eigenvector, sign: max |.| component > 0
void host_group_stats_test(cge_ctx *c, const i32 *ids, const i32 *task_row_off, i64 T, const unsigned char *side, const double *mean_in,
                           double *mean, double *sw, double *cov, double *vec, double *z, double *sums);
void host_group_cut_test(cge_ctx *c, const i32 *ids, const i32 *task_row_off, i64 T, int method, const double *z, int force_generic,
                         i32 *rc, i32 *nlow, i32 *children, double *vlow, double *vhigh, double *cmeans, i32 *route, i32 *ties);
// diameter_host.cpp
// the exact diameter of the resident embedding by brute force over this rank's share of the pair tiles (NaN for a non-finite
// embedding); `ai` / `aj` (optional): a pair attaining it, 1-based
double host_diameter_brute(cge_ctx *c, int part, int nparts, i64 *ai, i64 *aj);
// the same by landmark-pair pruning (brute force where the bounds prune too little), the largest of the ranks' shares:
// `lemb` = N landmark centroids (device, row-major), `lweight` their weights (device), `lcomm` their communities (0-based, C)
double host_diameter_landmarks(cge_ctx *c, const double *lemb, const double *lweight, const std::vector<i32> &lcomm, i64 C, i64 N);
void host_diameter_bounds_test(cge_ctx *c, const i64 *v2l, i64 N, const i64 *lcomm1, i64 C, int pass, double *P, i64 *nref_out,
                               int *pass_ran, double *ref_out, double *mean_out);
void host_ref_dist2_test(cge_ctx *c, const double *refs, i64 nref, double *rd2, double *mean_out);
void host_ensure_centred(cge_ctx *c); // Xc / rnorm: the centred feature-major copy of the resident embedding (made on first demand)
// link_host.cpp: what the cge_link_* entry points do, and the sweep's side of cge_link_fit
static inline void link_drop(cge_ctx *c) {
    c->link.valid = false; c->link.keys_ready = false; c->link.excl_ready = false; c->link.fib_ready = false; c->link.lf_ready = false;
    // cge_link_moments' scratch (an operand as large as Xc, partials of O(n * blocks)) goes with the model
    c->link.mXp.release(); c->link.mrp.release(); c->link.mf.release(); c->link.mrow.release(); c->link.mbin.release();
    c->link.mout.release();
    // and cge_link_triangles' (Q is 8 tld^2 bytes)
    c->link.tQ.release(); c->link.tpart.release(); c->link.tout.release(); c->link.tokeys_in.release(); c->link.tokeys.release();
    c->link.tlong.release(); c->link.tdeg.release(); c->link.ttri.release(); c->link.toff.release();
}
// a sweep that cge_link_fit runs calls this when alpha has just become the best of the wanted kind: Ta / Tb (N each, the sweep's
// numbering; old2new un-permutes a relabelled sweep) are copied aside on the stream
void link_capture(cge_ctx *c, const double *Ta, const double *Tb, i64 N, const i32 *old2new, double alpha);
void host_link_fit(cge_ctx *c, const cge_score_args *a, int which, double out[7], int *out_len, cge_trace *trace);
void host_link_set_model(cge_ctx *c, int directed, double alpha, double hi, const double *f_out, const double *f_in, i64 n);
void host_link_model_fetch(cge_ctx *c, int *directed, double *alpha, double *hi, double *f_out, double *f_in, double *T_out,
                           double *T_in, int64_t *N);
void host_link_prob(cge_ctx *c, const int64_t *i, const int64_t *j, i64 P, double *out);
void host_link_topk(cge_ctx *c, const int64_t *queries, i64 Q, i64 k, int exclude_edges, int64_t *out_j, double *out_p,
                    int64_t *out_cnt);
void host_link_rank(cge_ctx *c, const int64_t *i, const int64_t *j, i64 P, int exclude_edges, int64_t *out_greater,
                    int64_t *out_ties, int64_t *out_cand, double *out_p);
void host_link_auc(cge_ctx *c, int part, int nparts, int64_t *out_less, int64_t *out_ties, double *out_p, int64_t *n_neg,
                   double summary[3]);
void host_link_moments(cge_ctx *c, int diag, double *deg_out, double *deg_in, double *B, double *V, double *Cobs, int64_t *n_comm);
void host_link_triangles(cge_ctx *c, double *tri_exp, double *wed_exp, int64_t *tri_obs, int64_t *wed_obs, double summary[4]);
void host_link_triangles_q(cge_ctx *c, double *Q_out, i64 ld); // cge_link_triangles_test: Q of n <= 2048 vertices, copied out
// U != nullptr: cge_link_sample_test (n x n host doubles in the place of the counter stream)
void host_link_sample(cge_ctx *c, i64 seed, i64 stream_id, i64 cap, int64_t *out_i, int64_t *out_j, double *out_p, int64_t *n_edges,
                      const double *U, int directed_layout);
// score_host.cpp
struct cge_landmark_graph_io;
void host_landmark_graph_test(cge_ctx *c, cge_landmark_graph_io *io);
// wgcl_host.cpp
// ---- the packed form of an exact sweep's matrix: the NT = Nt (Nt + 1) / 2 upper 64 x 64 tiles (Nt = ceil(N / 64)), 4096 doubles
// each, in row-major order of the upper triangle (fit_symtile_kernel's numbering of t).  Diagonal tiles are stored whole, elements
// outside the matrix are 0.  Inside a tile the fit's lane 8 rq + cq owns the 8 x 8 block of rows 8 rq.., columns 8 cq..; the
// element (a, b) of that block sits at ((4 a + b / 2) * 64 + lane) * 2 + b % 2, so that each of the fit's 32 two-double loads is
// one contiguous kilobyte over the wave.  Every producer and consumer -- device and host -- addresses the buffer through these.
#define CGE_TILE_DOUBLES 4096
__host__ __device__ inline i64 cge_upper_tile(i64 I, i64 J, i64 Nt) { return I * Nt - I * (I - 1) / 2 + (J - I); } // I <= J
__host__ __device__ inline int cge_tile_slot(int r, int q) { // row r, column q of the tile
    const int lane = 8 * (r >> 3) + (q >> 3), a = r & 7, b = q & 7;
    return ((4 * a + (b >> 1)) * 64 + lane) * 2 + (b & 1);
}
// element (i, j) of the symmetric matrix; below the diagonal tiles the mirrored element (j, i) is the one stored
__host__ __device__ inline i64 cge_packed_index(i64 i, i64 j, i64 Nt) {
    if ((i >> 6) > (j >> 6)) { const i64 s = i; i = j; j = s; }
    return cge_upper_tile(i >> 6, j >> 6, Nt) * CGE_TILE_DOUBLES + cge_tile_slot((int)(i & 63), (int)(j & 63));
}
// tile t of the row-major upper triangle -> (I, J): start(I) = I Nt - I (I - 1) / 2
__host__ __device__ inline void cge_upper_tile_of(i64 t, i64 Nt, i64 &I, i64 &J) {
    const double bb = 2.0 * (double)Nt + 1.0;
    I = (i64)((bb - sqrt(bb * bb - 8.0 * (double)t)) * 0.5);
    if (I < 0) I = 0;
    if (I > Nt - 1) I = Nt - 1;
    while (I + 1 < Nt && (I + 1) * Nt - (I + 1) * I / 2 <= t) I++;
    while (I > 0 && I * Nt - I * (I - 1) / 2 > t) I--;
    J = I + (t - (I * Nt - I * (I - 1) / 2));
}
// ---- counter-based RNG of the sampler (splitmix64 finaliser over a 4-word counter): the same stream on host and device
__host__ __device__ inline uint64_t cge_sm64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}
__host__ __device__ inline uint64_t cge_ctr_rand(uint64_t seed, uint64_t stream, uint64_t k, uint64_t attempt, uint64_t which) {
    uint64_t h = cge_sm64(seed ^ 0x6a09e667f3bcc909ULL);
    h = cge_sm64(h ^ (stream * 0xd1342543de82ef95ULL + 1));
    h = cge_sm64(h ^ (k * 0x2545f4914f6cdd1dULL + 2));
    h = cge_sm64(h ^ (attempt * 0x9e6c63d0676a9a99ULL + 3));
    return cge_sm64(h ^ (which + 4));
}
// uniform integer in [0, range): multiply-high (bias < range / 2^64)
__host__ __device__ inline uint64_t cge_bounded(uint64_t r, uint64_t range) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(r, range);
#else
    return (uint64_t)(((__uint128_t)r * range) >> 64);
#endif
}
// positive / non-edge draws of one sample set on the device (kernels_fit.hip); 0-based i32 outputs of S entries
void k_draw_samples_dev(cge_ctx *c, i64 seed, i64 stream_id, i64 S, int directed, i32 *d_pos, i32 *d_ni, i32 *d_nj);
// the same in two halves: _begin enqueues the draws and the first round of the rejection and returns (no synchronisation);
// _finish looks at the round's verdict and runs whatever rounds are left (a local edge list only: no exchange in between)
void k_draw_samples_begin(cge_ctx *c, i64 seed, i64 stream_id, i64 S, int directed, i32 *d_pos, i32 *d_ni, i32 *d_nj);
void k_draw_samples_finish(cge_ctx *c);
void k_prep_samples(cge_ctx *c, const i32 *pos, const i32 *pos_pairs, const i32 *ni_in, const i32 *nj_in, const i32 *e_src,
                    const i32 *e_dst, const double *e_w, i64 S, int directed, i32 *pi, i32 *pj, i32 *ni, i32 *nj, double *wts);
void host_draw_samples(cge_ctx *c, i64 seed, i64 stream_id, i64 S, int directed, i64 *pos_idx, i64 *neg_i, i64 *neg_j);
void host_pos_draw(i64 seed, i64 stream_id, i64 S, i64 m, i64 *pos_idx);
bool sampler_uses_device(const cge_ctx *c); // large resident graph: the sampler runs on the device
struct OrigView { // original graph pieces needed in landmark mode (device, 0-based)
    i64 n = 0, m = 0;
    const double *Xr = nullptr;
    const double *vw = nullptr;
    const i32 *v2l = nullptr;
    const double *lweight = nullptr; // == score graph vweights
    const i32 *src = nullptr, *dst = nullptr;
    const double *h_w = nullptr; // host edge weights
    double hi = 0.0;             // diameter
    const i32 *h_lcomm = nullptr; // host copy of the landmarks' communities (the score graph's G.comm), when the caller has one
};
// What a landmark-mode sweep on the fused path has prepared when cge_score_batch takes it over instead of running it
// (host_wgcl_sweep with `defer`): the buffers the fused fit, vect_B and JS read, moved out of the context (their device
// pointers stay valid), and the host copy of the epilogue tables (auc_part is re-pointed by the batch).
struct SweepHandoff {
    int max_G = 0;          // (set by the batch) a fit of more workgroups shares no launch: the sweep runs as cge_score's
    bool deferred = false;
    i64 N = 0, C = 0, S = 0, n_sets = 0, Tld = 0;
    int split = 0;
    FlowGeometry geo{}; // the geometry of its fit
    DevBuf<double> Lh, vw, bt_part, vectC, T, fused_pw;
    DevBuf<float> Ll;
    DevBuf<i32> comm, bt_fc, bt_ns, bt_base, cm_off;
    std::vector<std::unique_ptr<DevSamples>> dsets;
    std::vector<cge_fit_fused> h_epi;
    const double *w = nullptr; // the fit's targets (inside `vw`)
    // A directed member (landmark mode, >= 256 landmarks; its fit shares fit_flow_dir_multi_kernel's launch): the normalised D
    // and, under pow_exp2, its row-major logarithm (Lh / Ll above; `logs`), a power matrix of its own, Tin / Tout (Tio: N each)
    // and the in- / out-degrees (deg: N each), the community tables, and the landmark state the local score reads (v2l, lweight).
    // bvec_form: the form of k_bvec its own sweep picks (the context's layout flags are the next member's by then).
    bool directed = false, logs = false;
    int bvec_form = 0;
    DevBuf<double> D, GD, Tio, deg, lweight;
    DevBuf<i32> cm_mem, cm_pos, v2l;
};
// The alpha bookkeeping of one sweep, the reference's (src/divergence.jl:35-38, :213-223, :242-253, :256): the patience counters,
// the skip flags and the best values.  host_wgcl_sweep keeps one, host_batch_sweep one per member (wgcl_host.cpp).
struct AlphaBook {
    static constexpr double delta = 0.001, AlphaMax = 10.0, AlphaStep = 0.25; // :35-37 / :288-290
    static constexpr i64 n_alpha = (i64)((AlphaMax + delta) / AlphaStep + 1e-9); // alpha = ia AlphaStep, ia = 1 .. n_alpha
    int div_counter = 5, auc_counter = 5; // :38
    bool skip_div = false, skip_auc = false;
    double best_div, best_div_ext, best_div_int, best_auc_err, best_auc, best_alpha = -1.0, best_alpha_auc = -1.0;
    i64 S;             // samples of the local score (its error bar, :217)
    int split;         // --split-global: the divergence is the mean of the internal and external ones
    cge_trace *trace;  // optional; emptied by the constructor, one entry per alpha taken (at most 64)
    AlphaBook(i64 S_, int split_, cge_trace *trace_);
    // the sweep may end at this alpha (both counters at their last value, or done): the next alpha is not enqueued ahead
    bool may_end_here() const { return (skip_div || div_counter == 1) && (skip_auc || auc_counter == 1); }
    bool ended() const { return skip_div && skip_auc; } // :253
    // one alpha's scalars (laid out RES_*, fitted in `iters` iterations): the block partials added in block order, then the AUC's
    // counter and best values, the divergence's, the trace
    void take(const double *res, double alpha, i64 iters);
    void write(double out[7], int *out_len) const; // the reference's 7-vector (:256)
};
struct cge_local_score_io; // (include/cge_hip_testing.h)
void host_local_score_test(cge_ctx *c, cge_local_score_io *io); // the testing hook of the local score's stages (sweep_hooks.cpp)
struct cge_vect_b_problem; // (include/cge_hip_testing.h)
void host_packed_gd_test(cge_ctx *c, const double *emb, const double *diag, i64 N, i64 d, double alpha, int pow_method, double *lo_hi,
                         double *GD);
struct cge_sweep_setup_io; // (include/cge_hip_testing.h)
void host_sweep_setup_test(cge_ctx *c, cge_sweep_setup_io *io); // the testing hook of the sweep's set-up (sweep_hooks.cpp)
// the directed degree pass of a score graph given as an edge list (score_host.cpp): c->s_degin / s_degout and the star counts
void edge_degrees(cge_ctx *c, const i32 *src, const i32 *dst, const double *w, i64 m, i64 N, DevBuf<i32> &star);
struct cge_fit_problem; // (include/cge_hip_testing.h)
struct cge_fused_chain_problem; // (include/cge_hip_testing.h)
void host_fused_chain_test(cge_ctx *c, cge_fused_chain_problem *probs, int n, double eps,
                           double delta); // the testing hook of the fused chain's epilogue (sweep_hooks.cpp)
void host_fit_test(cge_ctx *c, cge_fit_problem *probs, int n, int directed, int form, double eps, double delta,
                   int *form_ran); // the testing hook of the Chung-Lu fit's forms (sweep_hooks.cpp)
void host_vect_b_test(cge_ctx *c, const cge_vect_b_problem *p1, const cge_vect_b_problem *p2, int directed, int form,
                      int landmarks, int n_modes, int *form_ran); // the testing hook of vect_B's forms (sweep_hooks.cpp)
void host_wgcl_sweep(cge_ctx *c, const ScoreGraph &G, const OrigView *orig, const i32 *ex_src, const i32 *ex_dst,
                     const double *ex_hw, i64 ex_m, int directed, int split, const SampleSet &smp, double out[7],
                     int *out_len, cge_trace *trace, SweepHandoff *defer = nullptr);
// cge_score_batch's launch groups: members in order, a group closes when the next member's G would take the sum beyond
// `cus` or its NW differs; group_of[k] = the group of member k (-1: not batched, G[k] <= 0).  Returns the number of groups.
bool batch_group_closes(int g_sum, int g_nw, int g_size, int G, int NW, int cus);
// one member of a batch whose sweep was handed over: its outputs, and `redo` = its persistent fit was abandoned (the batch
// scores it again on its own, through cge_score's path)
struct BatchMember {
    SweepHandoff h;
    double *out = nullptr;
    int *out_len = nullptr;
    cge_trace *trace = nullptr;
    bool redo = false;
};
// the alpha sweeps of one launch group in lock-step (sum of G <= CUs, one NW, at most CGE_BATCH_MAX members; all members
// undirected or all directed)
void host_batch_sweep(cge_ctx *c, std::vector<BatchMember *> &group);
int score_batch_run(cge_ctx *c, const cge_score_args *a, const cge_embedding_view *views, i64 K, const char *who, double *out,
                    int *out_len, cge_trace *traces);
// score_host.cpp: what the entry points of the same names (cge_*) do
struct LandmarkRun { // cge_landmarks_run's arguments; need_wedges: build the N x N landmark-pair matrix too (else on first demand)
    const i64 *cl_flat, *cl_off;
    i64 ncl, land, forced; // (land: once lm_clamp has run, clamped to the unique rows)
    int method, directed;
    bool need_wedges;
    double t0 = 0.0; // start of the phase being timed (c->phases)
};
LandmarkRun score_landmark_run(const cge_ctx *c, const cge_score_args *a); // the landmark run of a cge_score
void host_landmarks_run(cge_ctx *c, LandmarkRun R);
void host_landmarks_info(cge_ctx *c, const char *who = "landmarks_info"); // the last run's landmark-pair matrix, built on first demand
void host_landmarks_fetch(cge_ctx *c, double *dii, double *embed, int64_t *cluster, int64_t *ledges, double *lw_e, double *lweight,
                          int64_t *v_to_l);
void host_score(cge_ctx *c, const cge_score_args *a, double out[7], int *out_len, cge_trace *trace, SweepHandoff *defer,
                bool reuse_samples); // `defer` / `reuse_samples`: a member of cge_score_batch
void host_wgcl(cge_ctx *c, const cge_wgcl_args *a, double out[7], int *out_len, cge_trace *trace);
void host_js(cge_ctx *c, const double *vC, const double *vB, i64 len, const uint8_t *vI, int internal, double *out);
void host_edge_scatter(cge_ctx *c, const int64_t *v_to_l, i64 N, i64 C, int directed, i64 e0, i64 e1, double *wedges_out,
                       double *vect_C_out);
