#!/usr/bin/env python3
"""bench.py -- edge-alpha evaluations/s of the divergence-scoring hot path on MI355X.

One step = example/CGE_CLI.jl:10-24 on device-resident inputs (cge_score): landmarks()
(runsplit + aggregation + per-edge scatter) followed by wGCL() in landmark mode (diameter of the
original embedding, landmark distance matrix, 40-step alpha sweep with Chung-Lu fit, JS and local
score).  metric = m * A / T  (m original edges, A alphas evaluated, T wall time per step).

  python bench.py --gpus 1 --steps 3 --warmup 1
  python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs bench_out   # + the last step's outputs, bench_out/<name>.npy
  python bench.py --full                                                    # + roofline, CPU baseline, other configurations
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
      bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the steps, writes the outputs if asked and prints the line.  Everything else it can
measure (per-kernel event timers and the roofline, the back-to-back scatter, the CPU baseline, the other BASELINE
configurations, N > 1: one embedding per GPU) runs with --full only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # BASELINE.json "metric": 10M-edge d=128 ABCD graph ("headline metric" row)
    "headline": dict(n=1_000_000, m=10_000_000, C=500, d=128, land=4000, forced=4, method="rss", samples=10000),
    # configs[1]: ABCD 100k nodes / 1M edges, d=64, -l 400 -m rss2
    "cfg2": dict(n=100_000, m=1_000_000, C=50, d=64, land=400, forced=4, method="rss2", samples=10000),
    # configs[2]: ABCD 1M nodes / 20M edges, d=128, -l 4000 -m diameter (its 8-GPU sharding is the driver's N=8 run)
    "cfg3": dict(n=1_000_000, m=20_000_000, C=500, d=128, land=4000, forced=4, method="diameter", samples=10000),
    # config 3's graph under the `size` rule (the fourth split rule at full size; parity fixture oracle_cfg3_size.npz)
    "cfg3_size": dict(n=1_000_000, m=20_000_000, C=500, d=128, land=4000, forced=4, method="size", samples=10000),
    # configs[3]: directed 1M-node graph, d=128, --samples-local 1000000, automatic landmarks max(4 sqrt(n), 4C)
    "cfg4": dict(n=1_000_000, m=10_000_000, C=500, d=128, land=4000, forced=4, method="rss", samples=1_000_000,
                 directed=True),
    # configs[4]: ABCD 10M nodes / 200M edges, d=512, -l 12000 (fp32-MFMA bound pass of the diameter).  The 41 GB embedding
    # is generated on the device and handed over as a device pointer (cge_set_embedding_device); --scale shrinks n and m.
    "cfg5": dict(n=10_000_000, m=200_000_000, C=1500, d=512, land=12000, forced=4, method="rss", samples=10000,
                 device_embedding=True),
    # config 5's own shape at the size its oracle fixture exists for (tests/golden/oracle_cfg5_200k.npz: 12 000 landmarks at
    # d = 512 on 200 000 vertices; `m_exact`: the edge count asked of the generator, not m x 1.05)
    "cfg5_200k": dict(n=200_000, m=4_000_000, m_exact=4_200_000, C=1500, d=512, land=12000, forced=4, method="rss", samples=10000),
    "small": dict(n=50_000, m=500_000, C=25, d=128, land=200, forced=4, method="rss", samples=10000),
}
F64_MFMA_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix peak (AMD datasheet; MI355X_MICROARCH.md lists no f64 row)
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: f32-input MFMA = the fp32 vector peak (155 TF measured)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: bf16 dense MFMA ~2.5 PFLOP/s
HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def cpu_baseline(g, wl, budget_vertices=60000):
    """The oracle (single-thread C restatement of the reference) on a bounded sample of the SAME graph:
    the sub-graph induced by the first communities (~budget_vertices vertices), landmarks scaled by the
    same ratio; call shape = landmarks() then wGCL(..., v_to_l = Int[]) on the landmark graph
    (test/runtests.jl:95-96; BASELINE.md item 5: the reference cannot build its O(n^2) objects here)."""
    from oracle import oracle as orc

    comm = g["comm"][:, 0]
    sizes = np.bincount(comm)[1:]
    k = int(np.searchsorted(np.cumsum(sizes), budget_vertices)) + 1
    k = max(2, min(k, len(sizes)))
    keep = comm <= k
    newid = np.cumsum(keep)  # 1-based ids of the kept vertices
    e = g["edges"]
    em = keep[e[:, 0] - 1] & keep[e[:, 1] - 1]
    edges = np.asfortranarray(np.stack([newid[e[em, 0] - 1], newid[e[em, 1] - 1]], axis=1))
    ew = g["eweights"][em]
    n_s = int(keep.sum())
    vw = np.zeros(n_s)
    np.add.at(vw, edges[:, 0] - 1, ew)
    np.add.at(vw, edges[:, 1] - 1, ew)
    ok = vw > 0  # the induced sub-graph may isolate a few vertices: give them a unit weight instead of dropping
    vw[~ok] = 1.0
    emb = np.asfortranarray(g["embedding"][keep])
    cm = np.asfortranarray(comm[keep].reshape(-1, 1))
    clusters = [np.flatnonzero(cm[:, 0] == c) + 1 for c in range(1, k + 1)]
    land = max(4 * k, int(round(wl["land"] * n_s / g["n"])))
    rng = np.random.default_rng(42)
    t0 = time.perf_counter()
    dii, lemb, lcomm, ledges, lw, lweight, v2l = orc.landmarks(edges, ew, vw, clusters, cm, emb, False, land,
                                                               wl["forced"], wl["method"], False)
    N = len(dii)
    S = wl["samples"]
    pos = rng.integers(1, len(lw) + 1, size=(1, S))
    ni = rng.integers(1, N + 1, size=(1, S))
    nj = rng.integers(1, N + 1, size=(1, S))
    nj[ni == nj] = nj[ni == nj] % N + 1
    res, tr = orc.wGCL(ledges, lw, lcomm, lemb, dii, lweight, [], [], np.zeros((0, 2), np.int64), [],
                       np.zeros((0, 0)), False, (pos, ni, nj), trace=True)
    t = time.perf_counter() - t0
    A = len(tr["iters"])
    return {"value": len(ew) * A / t, "unit": "edge-alpha evals/s", "cores": 1, "kind": "port",
            "sample": f"oracle (oracle/cge_oracle.c, 1 thread) on the sub-graph induced by the first {k} communities "
                      f"of the bench graph: n={n_s}, m={len(ew)}, d={emb.shape[1]}, {N} landmarks; landmarks() + "
                      f"wGCL(v_to_l=Int[]) on the landmark graph, {A} alphas, {t:.1f} s"}


ROOFLINE_KERNELS = ("fit_persistent", "fit_symv", "group_stats", "group_project", "sorted_prefix", "pcent", "pair_list",  # (pcent: also the bf16 form)
                    "max_pair_dist", "edge_scatter", "edge_scatter_wedges", "rss2_walk", "group_eig")


def full_size_oracle(workload):
    """The oracle's own FULL-SIZE run of this workload, as recorded in the provenance of its committed fixture
    (tests/golden/oracle_<workload>.npz, written by make_oracle_fixture_*.py on the build container, one core): seconds of
    landmarks() + wGCL*() and the evals/s they amount to.  Not timed here (7-13 CPU-minutes); reported beside the bounded
    sample that is."""
    import re

    path = os.path.join(ROOT, "tests", "golden", f"oracle_{workload}.npz")
    if not os.path.exists(path):
        return None
    fx = np.load(path, allow_pickle=False)
    prov = str(fx["provenance"])
    mt = re.search(r"landmarks (\d+) s(?:,| \+) (?:score|wGCL) (\d+) s", prov)
    if not mt:
        return None
    t_lm, t_sc = float(mt.group(1)), float(mt.group(2))
    A, m = len(fx["iters"]), int(fx["m"])
    return {"landmarks_s": t_lm, "wgcl_s": t_sc, "alphas": A, "m": m, "value": m * A / (t_lm + t_sc),
            "where": "build container, 1 core, oracle/cge_oracle.c; diameter handed in from tests/diameter_ref.py where the "
                     "provenance says so (the reference's O(n^2 d) loop is not runnable at this size)", "provenance": prov}


DUMP_BUDGET_BYTES = 60 << 20  # all arrays of --dump-outputs together (npy headers aside): under 64 MB


def dump_outputs(path, arrays):
    """`arrays`: name -> array, written as <path>/<name>.npy in float64 (ids and counts included: exact below 2^53).  Each
    array may take an equal share of DUMP_BUDGET_BYTES; a larger one is replaced by a fixed, seeded sample of its rows, in
    order (the same rows in every run of the same shape)."""
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BUDGET_BYTES // 8 // len(arrays)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        if a.size > cap:
            rows = max(1, cap // (a.size // a.shape[0]))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], rows, replace=False))]
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a))


def _crc(a):
    import zlib

    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def measure_other_config(name, seed, steps, warmup, dev):
    """One more BASELINE configuration on the driver's clock: fresh context, one upload (timed), `warmup`
    untimed and `steps` timed scores of the SAME step the headline runs (landmarks() incl. the N x N landmark-pair matrix +
    wGCL*() in landmark mode, inputs resident), then -- outside the timed region -- the result and the raw landmark ids
    against the committed full-size oracle fixture tests/golden/oracle_<name>.npz (elements 1-4 at 1e-9, CRC of v_to_l)."""
    import torch

    from cge.jl_amd import api, synth

    wl = dict(WORKLOADS[name])
    directed = bool(wl.get("directed", False))
    dev_emb = bool(wl.get("device_embedding", False))
    t0 = time.perf_counter()
    g = synth.abcd_like(wl["n"], wl.get("m_exact") or int(wl["m"] * 1.05), wl["C"], 1 if dev_emb else wl["d"], seed=seed, directed=directed)
    t_gen = time.perf_counter() - t0
    ctx = api.Context(dev.index or 0)
    try:
        if dev_emb:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed)
            centres = torch.randn(g["C"], wl["d"], generator=gen, device=dev, dtype=torch.float64) * 2.0
            comm_dev = torch.from_numpy(g["comm"][:, 0] - 1).to(dev)
            X = torch.empty(g["n"], wl["d"], dtype=torch.float64, device=dev)
            for a in range(0, g["n"], 1 << 20):
                b = min(g["n"], a + (1 << 20))
                X[a:b] = centres[comm_dev[a:b]] + torch.randn(b - a, wl["d"], generator=gen, device=dev, dtype=torch.float64) * 0.5
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.set_graph(g["edges"], g["eweights"], g["n"])
            ctx.set_embedding_device(X.data_ptr(), g["n"], wl["d"], row_major=True)
            ctx.set_vertex_data(g["comm"], g["vweights"])
            t_upload = time.perf_counter() - t0
            del X, comm_dev
            torch.cuda.empty_cache()
        else:
            t0 = time.perf_counter()
            ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
            t_upload = time.perf_counter() - t0
        ctx.set_option("landmark_edges", 1)

        def step():
            return ctx.score(g["clusters"], wl["land"], wl["forced"], wl["method"], directed=directed, seed=seed,
                             auc_samples=wl["samples"])

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = step()
        torch.cuda.synchronize()
        sec = (time.perf_counter() - t0) / steps
        A = ctx.last_trace["n_alpha"]
        ent = {"ms_per_step": round(sec * 1e3, 4), "steps": steps, "warmup": warmup, "value": g["m"] * A / sec,
               "value_incl_h2d": g["m"] * A / (sec + t_upload), "upload_s": round(t_upload, 4), "alphas_evaluated": A,
               "n": g["n"], "m": g["m"], "d": wl["d"], "landmarks": int(ctx.get_stat("landmarks")),
               "flags": f"-l {wl['land']} -f {wl['forced']} -m {wl['method']}" + (" -d" if directed else "")
                        + f" --samples-local {wl['samples']}",
               "phases_ms": {k: round(v, 3) for k, v in ctx.phase_ms().items()},
               "result": [float(x) for x in res], "matches_fixture": None, "gen_s": round(t_gen, 1)}
        fpath = os.path.join(ROOT, "tests", "golden", f"oracle_{name}.npz")
        if os.path.exists(fpath) and seed == 42:
            fx = np.load(fpath, allow_pickle=False)
            v2l = ctx.landmarks_fetch()[6].astype(np.int32)
            ids_ok = (np.array_equal(v2l, fx["v_to_l"]) if "v_to_l" in fx else _crc(v2l) == int(fx["v_to_l_crc"]))
            exp = fx["result"]
            # elements 1-4 are deterministic given the partition; 5-7 depend on the draws (library-drawn here)
            sc_ok = bool(res[0] == exp[0] and np.allclose(res[1:4], exp[1:4], rtol=1e-9, atol=1e-15))
            ent["matches_fixture"] = bool(ids_ok and sc_ok)
            ent["fixture"] = {"file": f"tests/golden/oracle_{name}.npz", "v_to_l_crc_equal": bool(ids_ok),
                              "elements_1_4_within_1e-9": sc_ok}
        return ent
    finally:
        ctx.close()
        del g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)  # a step is ~33 ms at the headline: ten of them average out most of the jitter
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="headline", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: per-kernel event timers and the roofline, the "
                         "back-to-back scatter, the CPU baseline, the other BASELINE configurations, N > 1: one embedding per "
                         "GPU.  The --no-* options and --profile-all below act on these")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64): the score "
                         "vector, the per-alpha trace and, on one GPU, the landmark state (large arrays as a seeded sample)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--profile-all", action="store_true",
                    help="event timers around every kernel family (default: only the kernels priced against a roofline)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the workload's n and m (the line says the actual sizes)")
    ap.add_argument("--diameter", type=int, default=0, help="0 auto (pruned, brute-force fallback), 1 brute force, 2 pruned")
    ap.add_argument("--lazy-landmark-edges", action="store_true",
                    help="leave the N x N landmark-pair matrix / landmark edge count of landmarks() (src/landmarks.jl:433-463) out "
                         "of the timed step (an undirected score does not read it); default: the step builds it")
    ap.add_argument("--no-back-to-back", action="store_true",
                    help="skip the 30 back-to-back passes of the per-edge scatter behind the timed region (profiles of the step alone)")
    ap.add_argument("--no-independent", action="store_true",
                    help="N > 1: skip the second measurement (one embedding per GPU, no collective)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="N = 1 headline run: do not follow it with the other BASELINE configurations (cfg2, cfg3, cfg4; cfg5 when "
                         ">= 200 GB of HBM are free and the run is still inside --other-budget-s), reported as `other_configs`")
    ap.add_argument("--other-budget-s", type=float, default=240.0,
                    help="wall-clock budget of the whole bench.py run after which no further configuration is started")
    args = ap.parse_args()
    t_start = time.perf_counter()

    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        log(f"bench.py: --gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
        sys.exit(2)
    if not torch.cuda.is_available():
        log("bench.py: no GPU visible; the hot path has no CPU fallback")
        sys.exit(3)
    # CGE_REHEARSAL_ONE_GPU=1: every rank on cuda:0 with the gloo backend (functional rehearsal of the N > 1
    # path on a one-GPU box; never used for reported numbers)
    rehearsal = os.environ.get("CGE_REHEARSAL_ONE_GPU") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    import __graft_entry__ as ge
    from cge.jl_amd import api, synth

    if not os.path.exists(api.library_path()):
        if rank == 0:
            ge.build()
        if world > 1:
            dist.barrier()
    wl = dict(WORKLOADS[args.workload])
    if args.scale != 1.0:
        wl["n"], wl["m"] = max(1000, int(wl["n"] * args.scale)), max(10000, int(wl["m"] * args.scale))
    t0 = time.perf_counter()
    directed = bool(wl.get("directed", False))
    dev_emb = bool(wl.get("device_embedding", False))
    g = synth.abcd_like(wl["n"], wl.get("m_exact") or int(wl["m"] * 1.05), wl["C"], 1 if dev_emb else wl["d"], seed=args.seed, directed=directed)
    if rank == 0:
        log(f"[bench] synthetic ABCD-like graph: n={g['n']} m={g['m']} d={wl['d']} C={g['C']} ({time.perf_counter()-t0:.1f} s)")
    ctx = api.Context(local_rank)

    def upload():
        """The resident inputs of the score.  N > 1: called after the collectives are up, with option shard_ingest -- every
        rank uploads (and keeps) its slice of the edge list, and uploads its slice of the embedding's rows, which are then
        all-gathered device to device; `upload_s` is what one rank waits for."""
        if dev_emb:  # community centre + isotropic noise, as synth.abcd_like builds it, but in HBM (fp64, row-major)
            gen = torch.Generator(device=dev)
            gen.manual_seed(args.seed)
            centres = torch.randn(g["C"], wl["d"], generator=gen, device=dev, dtype=torch.float64) * 2.0
            comm_dev = torch.from_numpy(g["comm"][:, 0] - 1).to(dev)
            X = torch.empty(g["n"], wl["d"], dtype=torch.float64, device=dev)
            for a in range(0, g["n"], 1 << 20):
                b = min(g["n"], a + (1 << 20))
                X[a:b] = centres[comm_dev[a:b]] + torch.randn(b - a, wl["d"], generator=gen, device=dev, dtype=torch.float64) * 0.5
            torch.cuda.synchronize()
            g["d"], g["embedding"] = wl["d"], None
            t0 = time.perf_counter()
            ctx.set_graph(g["edges"], g["eweights"], g["n"])
            ctx.set_embedding_device(X.data_ptr(), g["n"], wl["d"], row_major=True)
            ctx.set_vertex_data(g["comm"], g["vweights"])
            t_upload = time.perf_counter() - t0
            del X, comm_dev
            torch.cuda.empty_cache()
        else:
            t0 = time.perf_counter()
            ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
            t_upload = time.perf_counter() - t0
        return t_upload

    t_upload = None
    if world == 1:
        t_upload = upload()
    ctx.set_option("diameter", args.diameter)
    ctx.set_option("landmark_edges", 0 if args.lazy_landmark_edges else 1)
    coll, coll_backend = None, None
    if world > 1:
        # default: the library's own RCCL communicator (ncclAllReduce on its stream, no host synchronisation per exchange);
        # CGE_COLLECTIVES=torch (or a failed init, or the one-GPU rehearsal) -> the torch.distributed hook
        # (CGE_REHEARSAL_TRY_RCCL=1: the one-GPU rehearsal walks through the handshake too -- RCCL refuses two ranks on one
        # device, so it exercises the agreed fall-back to the hook)
        if os.environ.get("CGE_COLLECTIVES", "rccl") == "rccl" and (not rehearsal or os.environ.get("CGE_REHEARSAL_TRY_RCCL") == "1"):
            # Every rank must take the same branch (ncclCommInitRank is collective): first agree that librccl loads and
            # hands out ids everywhere, then create the communicator, then agree that it exists everywhere.
            def all_ok(ok):
                flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                return bool(flag.item())

            uid, err = None, None
            try:
                uid = api.rccl_unique_id()
            except Exception as e:  # library missing / symbol missing
                err = e
            if all_ok(uid is not None):
                ids = [uid if rank == 0 else None]
                dist.broadcast_object_list(ids, src=0)
                try:
                    ctx.init_rccl(ids[0], rank, world)
                except Exception as e:
                    err = e
                if all_ok(err is None):
                    coll_backend = "in-library RCCL (ncclAllReduce on the ctx stream)"
                elif err is None:
                    ctx.finalize_rccl()
            if coll_backend is None:
                log(f"[bench] rank {rank}: in-library RCCL unavailable ({err!r}); using the torch.distributed hook")
        if coll_backend is None:
            from cge.jl_amd.dist import TorchCollectives

            coll = TorchCollectives(ctx, wl["land"] * wl["land"] * 2 + 1024, dev)
            coll_backend = "torch.distributed hook (" + dist.get_backend() + ")"

    if world > 1:
        ctx.set_option("shard_ingest", 0 if os.environ.get("CGE_SHARD_INGEST") == "0" else 1)
        # the embedding rows sharded by community: a rank uploads, keeps and splits the rows of its own communities only
        ctx.set_option("shard_rows", 0 if os.environ.get("CGE_SHARD_ROWS") == "0" else 1)
        fence0 = dist.barrier
        fence0()
        t_upload = upload()
        t = torch.tensor([t_upload], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t_upload = float(t.item())
    ingest_stats = (ctx.get_stat("edges_resident"), ctx.get_stat("edges_total"), ctx.get_stat("rows_resident"), ctx.get_stat("rows_total"))

    def step():
        return ctx.score(g["clusters"], wl["land"], wl["forced"], wl["method"], directed=directed, seed=args.seed,
                         auc_samples=wl["samples"])

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if rehearsal:
        # two processes on one GPU cannot both keep a co-resident persistent grid: use one launch per iteration
        ctx.set_option("fit_persistent", 1)
        log(f"[bench] rank {rank}: REHEARSAL mode (gloo, all ranks on cuda:0) -- numbers are not reportable")

    res = None
    for _ in range(args.warmup):
        res = step()
    # live HIP-event timers over the timed region: the kernels that carry a roofline entry (every timer is a pair of
    # events on the stream, about 4 us of serialisation each; --profile-all brackets every kernel family)
    # Inside the TIMED region only the timers of the fits run (the dominant kernel, whose live figure is the line's `roofline`);
    # the other roofline kernels are timed in a few extra, untimed steps behind it (TIMED_KERNELS / ROOFLINE_KERNELS below):
    # 60 event pairs per step were 0.25 ms of serialisation inside the number they were there to explain.
    # A plain run (no --full) keeps every timer off: its line carries no per-kernel figures.
    TIMED_KERNELS = ("fit_persistent", "fit_symv")
    if args.full:
        ctx.profile_select(() if args.profile_all else TIMED_KERNELS)
        ctx.profile_enable(True)
        ctx.profile_reset()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    prof = ctx.profile() if args.full else {}
    phases = ctx.phase_ms()
    trace = ctx.last_trace
    if args.dump_outputs and rank == 0:  # what the caller of the last timed score receives, before anything else runs
        # the trace marks an alpha whose divergence / AUC was no longer evaluated (that score's sweep had stopped) with NaN:
        # written as the evaluated values and a 0/1 mask of the alphas they belong to
        div_ok, auc_ok = ~np.isnan(trace["div"]), ~np.isnan(trace["auc"])
        outputs = {"result": res, "trace_iters": trace["iters"],
                   "trace_div": np.asarray(trace["div"])[div_ok], "trace_div_evaluated": div_ok,
                   "trace_auc": np.asarray(trace["auc"])[auc_ok], "trace_auc_evaluated": auc_ok}
        if world == 1:  # the landmark state that score left on the device (cge_landmarks_fetch)
            names = ("landmark_dii", "landmark_embedding", "landmark_community", "landmark_edges", "landmark_edge_weights",
                     "landmark_weights", "v_to_l")
            outputs.update(zip(names, ctx.landmarks_fetch()))
        dump_outputs(args.dump_outputs, outputs)
    if args.full and not args.profile_all:  # the other kernels that carry a roofline entry: the same step, a few more times, outside the timed region
        extra = 3 if args.workload != "cfg5" else 1
        ctx.profile_select(tuple(k for k in ROOFLINE_KERNELS if k not in TIMED_KERNELS))
        ctx.profile_reset()
        for _ in range(extra):
            step()
        fence()
        for name, p in ctx.profile().items():  # scaled to the timed region's step count (the per-step figures below divide by it)
            prof[name] = {"launches": p["launches"] * args.steps / extra, "total_ms": p["total_ms"] * args.steps / extra}
        ctx.profile_select(TIMED_KERNELS)
    # the per-edge scatter once more, back to back (the same live HIP-event timer): what the two kernels take when they follow
    # each other -- inside a step the pass starts cold (40 MB of edge words and the tables come from HBM behind the landmark
    # phase's traffic) and the timer also spans the gap between its two launches
    scatter_b2b = None
    if args.full and world == 1 and args.workload != "cfg5" and not args.no_back_to_back:
        try:
            ctx.profile_select(("edge_scatter",))
            ctx.profile_reset()
            for _ in range(30):
                ctx.edge_scatter(None, 1, g["C"], directed, want_wedges=False)
            pb = ctx.profile().get("edge_scatter")
            if pb and pb["launches"]:
                scatter_b2b = pb["total_ms"] / pb["launches"]
        except Exception as e:  # a measurement aid: never fail the bench line for it
            log(f"[bench] back-to-back scatter measurement skipped: {e!r}")
    stats_strong = None
    if world > 1:
        stats_strong = (coll.n_calls if coll is not None else ctx.get_stat("collective_calls"),
                        coll.bytes if coll is not None else ctx.get_stat("collective_bytes"))
    # N > 1, second measurement: ONE EMBEDDING PER GPU.  The path's natural multi-GPU use (comparing the embeddings of one
    # graph) has no exchange at all: every rank scores its own embedding of the resident graph, no collective, the job's
    # rate is the sum.  Reported beside the strong-scaling value of the contract, never instead of it.
    independent = None
    if args.full and world > 1 and not dev_emb and not args.no_independent:
        ctx.clear_collectives()
        rng = np.random.default_rng(args.seed + 7919 * (rank + 1))
        emb_r = np.asfortranarray(g["embedding"] + 0.05 * rng.standard_normal(g["embedding"].shape))
        ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], emb_r)
        del emb_r
        ctx.profile_enable(False)
        step()
        fence()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            res_i = step()
        fence()
        el = torch.tensor([time.perf_counter() - t1, float(ctx.last_trace["n_alpha"])], dtype=torch.float64, device=dev)
        tmax = el.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(el, op=dist.ReduceOp.SUM)
        sec_i = float(tmax[0].item()) / max(1, args.steps)
        independent = {"embeddings": world, "ms_per_step": sec_i * 1e3, "alphas_evaluated_sum": float(el[1].item()),
                       "value": g["m"] * float(el[1].item()) / sec_i, "unit": "edge-alpha evals/s",
                       "embeddings_per_s": world / sec_i, "scaling": "weak",
                       "note": "every rank scores its own embedding (the bench embedding + N(0, 0.05^2) noise, seeded per rank) "
                               "of the resident graph; no collective on the data path; value = m x (sum of the ranks' alphas) / "
                               "max over ranks of the step time"}
    if rank != 0:
        ctx.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    A = trace["n_alpha"]
    sec_per_step = elapsed / max(1, args.steps)
    value = g["m"] * A / sec_per_step

    def kern(name):
        p = prof.get(name, {"launches": 0, "total_ms": 0.0})
        return p["launches"], (p["total_ms"] / p["launches"] if p["launches"] else float("nan"))

    # Roofline per kernel: ALGORITHMIC work of one launch / average launch time measured
    # with HIP events on the library's stream.  The `roofline` object is the kernel with the largest total time.
    n, d, N = g["n"], g["d"], int(ctx.get_stat("landmarks"))
    hi, dpath, cand_pairs, cand_tiles = ctx.last_diameter()
    steps_prof = max(1, args.steps)
    work = {  # name -> (bound, peak, unit, algorithmic work per launch, note)
        "max_pair_dist": ("mfma", F64_MFMA_PEAK_TFLOPS, "TFLOP/s", 2.0 * d * (n * (n - 1) / 2) / world,
                          "fp64 MFMA, 2d flop per unordered vertex pair, all pairs"),
        "pcent": ("mfma", F32_MFMA_PEAK_TFLOPS, "TFLOP/s", 2.0 * d * n * max(1, ctx.get_stat("diameter_refs")),
                  "fp32 MFMA (v_mfma_f32_32x32x2_f32) upper bounds, 2d flop per (vertex, reference point) pair; reference "
                  "points = community centroids; priced against the f32-input MFMA peak"),
        "pcent_bf16": ("mfma", BF16_MFMA_PEAK_TFLOPS, "TFLOP/s", 3 * 2.0 * ((d + 31) // 32 * 32) * n * max(1, ctx.get_stat("diameter_refs")),
                       "upper bounds of the vertex-to-reference distances on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16) with "
                       "every operand split into two bf16 terms: three MFMAs per product (x.mu ~ xh.muh + xh.mul + xl.muh, rigorous "
                       "margin), so the work priced here is 3 x 2 K flop per (vertex, reference point) pair against the dense bf16 "
                       "peak; `algorithmic_f32_equivalent_tflops` = 2 d n C / t, what an f32-input pass of the same bounds would "
                       "have to sustain (its peak: 157.3).  The kernel is bound by the latency of fetching the reference tiles from "
                       "L2, not by the matrix pipe (profiles/r03_pcent_bf16_probe.txt)"),
        "pair_list": ("mfma", F64_MFMA_PEAK_TFLOPS, "TFLOP/s", None,
                      "fp64 MFMA, 2d flop per vertex pair of the candidate 128x128 tiles"),
        "fit_symv": ("hbm", HBM_PEAK_GBS, "GB/s", 8.0 * N * (N + 1) / 2,
                     "8 B per unordered landmark pair per Chung-Lu iteration"),
        "fit_persistent": ("hbm", HBM_PEAK_GBS, "GB/s", None,
                           "one launch = the whole Chung-Lu fit of one alpha with the matrix REGISTER-RESIDENT -- and, round 5, the "
                           "rest of the alpha's chain (power matrix in the prologue, vect_B tile sums and local-score tallies in "
                           "the epilogue: fit_flow_kernel<.., true>); algorithmic bytes = what that algorithm has to move through "
                           "memory: one read of the upper triangle of log2(1 - D) (a double and a float: 12 B per unordered "
                           "landmark pair; 8 B of GD where the chain is not fused) + per iteration the partial vectors written and read once (2 x Nt^2 x 64 "
                           "doubles), the iterate read by every tile (Nt(Nt+1)/2 x 128 doubles) and written once. The kernel "
                           "is latency-bound (two cross-workgroup hand-offs per iteration, DESIGN.md section 4), hence the low "
                           "fraction; `streaming_equivalent_gbs` = what a launch-per-iteration SYMV (SURVEY 8d(5): 8 B per "
                           "pair per iteration) would have to stream to match it -- a speed-up figure, not a roofline"),
        "group_stats": ("mfma", F64_MFMA_PEAK_TFLOPS, "TFLOP/s", None,
                        "covariance SYRK, priced as SURVEY 8(d)(3): |c| d^2 flop per split (the symmetric half at 2 flop per "
                        "entry) summed over the groups of a batch = rows x d^2; the timer also covers the means gather and the "
                        "chunk reduction"),
        "group_project": ("hbm", HBM_PEAK_GBS, "GB/s", None, "projection z: one 8d-byte row read per row of the batch"),
        "sorted_prefix": ("hbm", HBM_PEAK_GBS, "GB/s", None, "WSSE scan along sorted z: one 8d-byte row read per row of the batch"),
        "edge_scatter": ("hbm", HBM_PEAK_GBS, "GB/s", 24.0 * g["m"] / world,
                         "C x C cluster-pair scatter-add (edge pass + row reduction, kernels_scatter.hip), 24 B per edge "
                         "(2 x Int64 + Float64 as the reference stores them; the blocked device copy is 4 B per edge).  Steady "
                         "state on the blocked copy of the resident edge list: `first_call_ms` adds its one-off build "
                         "(`layout_build_ms`: key kernel + radix sort + gather + chunk table) paid by the first score of a graph"),
        "edge_scatter_wedges": ("hbm", HBM_PEAK_GBS, "GB/s", 24.0 * g["m"] / world,
                                "N x N landmark-pair scatter-add of landmarks() (src/landmarks.jl:433-451) incl. zeroing / writing "
                                "the N x N output and counting its positive entries: 24 B per edge as the reference stores them"),
        "rss2_walk": ("hbm", HBM_PEAK_GBS, "GB/s", None,
                      "rss2 rule (prefix / suffix RSS chains + merge): 2 x 8d bytes per row of the batch; the chains are "
                      "sequential in the rows of a group (the reference's order of additions) and pay an IEEE division per "
                      "row and column -- latency-bound by the longest group, not by HBM"),
        "group_eig": ("hbm", HBM_PEAK_GBS, "GB/s", None,
                      "batched principal eigenvector (Householder tridiagonalisation, matrix in registers for d <= 128): "
                      "8 d^2 bytes per matrix; 126 dependent steps per matrix -- latency-bound, not HBM-bound"),
    }
    kernels = {}
    if d <= 128 and "pcent" in prof and ctx.get_stat("diameter_bound_pass") == 2:  # the bf16-split bound pass ran under this timer
        prof["pcent_bf16"] = prof.pop("pcent")
    for name in prof:
        l_, ms_ = kern(name)
        ent = {"avg_launch_ms": ms_, "launches": int(round(l_)), "total_ms_per_step": prof[name]["total_ms"] / steps_prof,
               "timed_in": "the timed region" if (args.profile_all or name in TIMED_KERNELS) else "extra steps behind the timed region"}
        if name in work and l_:
            bound, peak, unit, w, note = work[name]
            if name == "pair_list":
                w = 2.0 * d * 128 * 128 * cand_tiles / max(1, l_ / steps_prof)
            if name in ("group_stats", "group_project", "sorted_prefix", "rss2_walk", "group_eig"):  # average batch of the last runsplit
                rows = ctx.get_stat("landmark_batch_rows") / max(1, ctx.get_stat("landmark_batches"))
                w = 1.0 * d * d * rows if name == "group_stats" else 8.0 * d * rows
                if name == "rss2_walk":
                    w = 16.0 * d * rows
                if name == "group_eig":
                    mats = ctx.get_stat("landmark_splits") / max(1, ctx.get_stat("landmark_batches"))
                    w = 8.0 * d * d * mats
                    if d > 128:  # panel form, matrix in memory: the 32 x 32 tiles on and below the diagonal are read once per
                        # step (both products of the symmetric pair from one read) and read + written once per panel of
                        # 8 steps = 8 B x d^3/3 x (1/2 + 1/8) per matrix -- this one IS bound by HBM
                        w = 8.0 * d ** 3 / 3.0 * 0.625 * mats
                        note = ("batched principal eigenvector, 128 < d <= 512: panel-blocked Householder tridiagonalisation with "
                                "the matrix in HBM; algorithmic bytes = half a read of the trailing block per step (lower tiles, "
                                "each serving both products of the symmetric pair) + half a read and write per panel of 8 steps "
                                "= 8 B x d^3/3 x 0.625 per matrix")
                ent["rows_per_launch"] = rows
            if name == "fit_persistent":  # iterations of the last step's sweep / its launches
                its = ctx.get_stat("fit_iterations") / max(1, l_ / steps_prof)
                Nt = (N + 63) // 64
                per_iter = 8.0 * (2 * Nt * Nt * 64 + Nt * (Nt + 1) // 2 * 128 + N) * (2 if directed else 1)
                # (the fused launch reads the stored logarithm, a double and a float per pair, instead of the power matrix)
                w = (12.0 if ctx.get_stat("fit_fused_alphas") > 0 else 8.0) * N * (N + 1) / 2 + its * per_iter
                ent["iterations_per_launch"] = its
                ent["streaming_equivalent_gbs"] = 8.0 * N * (N + 1) / 2 * its / (ms_ * 1e-3) / 1e9
            if name == "pcent_bf16":
                ent["algorithmic_f32_equivalent_tflops"] = 2.0 * d * n * max(1, ctx.get_stat("diameter_refs")) / (ms_ * 1e-3) / 1e12
            ach = w / (ms_ * 1e-3) / (1e12 if unit == "TFLOP/s" else 1e9)
            ent.update({"bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
                        "algorithmic_work_per_launch": w, "work_unit": "flop" if unit == "TFLOP/s" else "B",
                        "note": note})
        kernels[name] = ent
    # HBM traffic per launch from the committed PMC passes of this same command (profiles/run_profiles.sh)
    pmc = {}
    pmc_file = next((f for f in (os.path.join(ROOT, "profiles", f"r0{r}_pmc_traffic.json") for r in (5, 4, 3, 2, 1)) if os.path.exists(f)), "")
    kernel_of = {"fit_symv": ("fit_symtile_kernel", "fit_symreduce_kernel"), "fit_persistent": ("fit_flow_kernel",), "pcent": ("pcent_f32_rowres_kernel", "pcent_f32_kernel", "pcent_groups_kernel"),
                 "pcent_bf16": ("pcent_bf16_kernel", "pcent_groups_kernel"),
                 "pair_list": ("pair_list_kernel",), "edge_scatter": ("edge_pass_kernel", "edge_row_reduce_kernel"),
                 "edge_scatter_wedges": ("wedge_pass_kernel", "wedge_tile_kernel"),
                 "group_stats": ("group_cov_mfma_kernel", "group_cov_final_kernel", "gather_means_kernel"), "group_eig": ("group_eig_kernel",),
                 "max_pair_dist": ("max_pair_kernel",)}
    if args.full and os.path.exists(pmc_file) and args.workload == "headline" and world == 1:
        try:
            pmc = json.load(open(pmc_file))["kernels"]
        except Exception:
            pmc = {}
    for name, knames in kernel_of.items():  # template instances carry a <...> suffix in the profile; a timer may span two kernels
        hit = [k for k in pmc for kn in knames if k == kn or k.startswith(kn + "<")]
        if name in kernels and hit:
            kernels[name]["traffic"] = sum(pmc[k]["hbm_bytes_per_launch"] for k in hit)
    if "edge_scatter" in kernels:  # what the FIRST score of a resident graph pays on top: the blocked copy of the edge list
        build_ms = ctx.get_stat("edge_layout_build_us") / 1e3
        kernels["edge_scatter"]["layout_build_ms"] = build_ms
        kernels["edge_scatter"]["chunks"] = ctx.get_stat("edge_chunks")
        if scatter_b2b:
            kernels["edge_scatter"]["back_to_back_ms"] = scatter_b2b
            kernels["edge_scatter"]["back_to_back_frac"] = 24.0 * g["m"] / (scatter_b2b * 1e-3) / 1e9 / HBM_PEAK_GBS
        kernels["edge_scatter"]["first_call_ms"] = kernels["edge_scatter"]["avg_launch_ms"] + build_ms
    ranked = sorted((k for k in kernels if "frac" in kernels[k]), key=lambda k: -kernels[k]["total_ms_per_step"])
    dom = ranked[0] if ranked else None
    roofline = None
    if dom:
        e = kernels[dom]
        roofline = {"kernel": dom, "bound": e["bound"], "achieved": e["achieved"], "peak": e["peak"], "unit": e["unit"],
                    "frac": e["frac"], "traffic": e.get("traffic"), "avg_launch_ms": e["avg_launch_ms"],
                    "launches": e["launches"],
                    "algorithmic_work_per_launch": e["algorithmic_work_per_launch"], "note": e["note"]}
    out = {
        # `value`: m A / T with the inputs already resident in HBM when the timed region starts (the bench contract);
        # `value_incl_h2d`: SURVEY 8(d)'s T, which also pays one upload of the inputs (host arrays -> HBM) per score
        "metric": "edge_alpha_evals_per_sec", "value": value, "unit": "edge-alpha evals/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": sec_per_step * 1e3, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{args.workload}: ABCD-like n={n} m={g['m']} d={d} C={g['C']}, -l {wl['land']} "
                               f"-f {wl['forced']} -m {wl['method']} --seed {args.seed} --samples-local {wl['samples']}; "
                               f"landmarks() [clamp + runsplit + aggregation + per-edge scatter"
                               + (" + N x N landmark-pair matrix and its edge count" if (directed or not args.lazy_landmark_edges)
                                  else "; the N x N landmark-pair matrix of src/landmarks.jl:433-463 is NOT built (lazy)")
                               + f"; the landmark edge list stays on the device] + wGCL{'_directed' if directed else ''}() in "
                               "landmark mode [diameter of the original embedding, sample draws, D, 40-step alpha sweep], inputs "
                               "resident in HBM" + (" (embedding generated on the device)" if dev_emb else ""),
                   "n": n, "m": g["m"], "d": d, "communities": g["C"], "landmarks": N,
                   "alphas_evaluated": A, "parallelism": f"edges+pair-tiles sharded over {world} GPU(s)"},
        # SURVEY 8(d) puts the H2D copies inside T; the bench contract wants `value` with inputs already resident in HBM.
        # Both are reported: `value` = resident step, `value_incl_h2d` = m A / (step + one upload of the inputs).
        "value_incl_h2d": g["m"] * A / (sec_per_step + t_upload), "upload_s": t_upload,
        "ingest": ("every rank uploads everything" if world == 1 or ingest_stats[0] == ingest_stats[1]
                   else f"sharded: {ingest_stats[0]} of {ingest_stats[1]} edges and {ingest_stats[2]} of {ingest_stats[3]} embedding rows "
                        "resident on rank 0 (rows sharded by community when fewer than all: a rank uploads and keeps its own "
                        "communities' rows; else one slice per rank uploaded and all-gathered over xGMI)"),
        "rows_resident_rank0": ingest_stats[2], "rows_total": ingest_stats[3],
        "roofline": roofline, "kernels": kernels, "phases_ms": phases,
        "diameter": {"hi": hi, "path": dpath, "candidate_landmark_pairs": cand_pairs, "candidate_tiles": cand_tiles,
                     "all_landmark_pairs": N * (N + 1) // 2, "all_tiles": ((n + 127) // 128) * ((n + 127) // 128 + 1) // 2},
        "result": [float(x) for x in res],
    }
    if world > 1:
        calls, nbytes = stats_strong
        out["collectives"] = {"backend": coll_backend, "allreduce_calls_per_step": calls / (args.steps + args.warmup),
                              "bytes_per_step": nbytes / (args.steps + args.warmup)}
        if independent is not None:
            out["independent_embeddings"] = independent
    if args.full and world == 1 and not args.no_cpu_baseline and not directed and not dev_emb:
        try:
            out["cpu_baseline"] = cpu_baseline(g, wl)
            fs = full_size_oracle(args.workload) if args.scale == 1.0 else None
            if fs:
                out["cpu_baseline"]["full_size_oracle"] = fs
        except Exception as e:  # the baseline is reported, never required for the GPU number
            out["cpu_baseline"] = {"value": None, "unit": "edge-alpha evals/s", "cores": 1, "kind": "port",
                                   "sample": f"failed: {e!r}"}
    ctx.close()  # tear the context down before interpreter exit (profilers finalise their HIP hooks at exit)
    # The other single-GPU configurations of BASELINE.json on the same clock.  LAST key of the line: the driver keeps the
    # line's tail.  Headline `value` / `config` / `roofline` above are untouched by it.
    if args.full and world == 1 and args.workload == "headline" and args.scale == 1.0 and not args.no_other_configs:
        del g
        torch.cuda.empty_cache()
        other = {"headline": {"ms_per_step": round(sec_per_step * 1e3, 4), "steps": args.steps, "value": value,
                              "value_incl_h2d": out["value_incl_h2d"], "upload_s": round(t_upload, 4)}}
        for name, st, wu in (("cfg2", 10, 2), ("cfg3", 10, 2), ("cfg4", 10, 2), ("cfg5_200k", 3, 1), ("cfg5", 3, 1)):
            used = time.perf_counter() - t_start
            if used > args.other_budget_s:
                other[name] = {"skipped": f"time budget: {used:.0f} s of --other-budget-s {args.other_budget_s:.0f} used"}
                continue
            if name == "cfg5":
                free, _ = torch.cuda.mem_get_info()
                if free < 200e9:
                    other[name] = {"skipped": f"needs ~190 GB of free HBM ({free / 1e9:.0f} GB free)"}
                    continue
                if used > 0.5 * args.other_budget_s:
                    other[name] = {"skipped": f"time budget: {used:.0f} s used, cfg5 needs ~2 min (graph generation on the host)"}
                    continue
            try:
                other[name] = measure_other_config(name, args.seed, st, wu, dev)
                log(f"[bench] {name}: {other[name]['ms_per_step']:.2f} ms/step, matches_fixture={other[name]['matches_fixture']}")
            except Exception as e:  # never lose the headline line to a side measurement
                other[name] = {"failed": repr(e)}
        out["other_configs"] = other
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
