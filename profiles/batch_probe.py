#!/usr/bin/env python3
"""batch_probe.py -- K sequential cge_score calls against one cge_score_batch of the same K embeddings.

Per shape (n = 10^4 at -l 400, and config 2: 10^5 vertices, d = 64, -l 400 -m rss2) and K in 1, 4, 9, 16: end-to-end wall
time per member, the sweep per member (phase "sweep" of each separate score; phase "batch_sweep" / K for the batch), the
multi-problem fit launches and the member-alphas they fitted.  Every batch is checked against the separate scores (same bits)
before it is timed.  One JSON line per (shape, K) on stdout.

--directed: the same on directed graphs, where the members' fits alone share a launch (n = 10^4 at -l 400 and n = 10^5 at
-l 1000, d = 16): also the min .. max of every figure over the repetitions (the runs alternate: separate, batch, separate, ..)
and, with --fit-timers (a run of its own: the timers are event pairs on the stream), the device time of the fit kernels per
member (timers "fit_persistent" of the separate scores, "fit_batched" of the batch).  With K = 1 nothing is shared and the batch's sweep is the member's own phase "sweep".

    python profiles/batch_probe.py [--reps 3] [--shapes n1e4,cfg2] [--ks 1,4,9,16] [--directed [--fit-timers]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "n1e4": dict(n=10_000, m=100_000, C=20, d=64, land=400, method="rss"),
    "cfg2": dict(n=100_000, m=1_050_000, C=50, d=64, land=400, method="rss2"),
}
DIRECTED_SHAPES = {
    "n1e4": dict(n=10_000, m=100_000, C=20, d=16, land=400, method="rss"),
    "n1e5": dict(n=100_000, m=1_000_000, C=50, d=16, land=1000, method="rss"),
}


def embeddings(X, K, seed):
    rng = np.random.default_rng(seed)
    return [X] + [np.asfortranarray(X + 0.1 * k * rng.standard_normal(X.shape)) for k in range(1, K)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="n1e4,cfg2")
    ap.add_argument("--ks", default="1,4,9,16")
    ap.add_argument("--directed", action="store_true")
    ap.add_argument("--fit-timers", action="store_true", help="--directed: time the fit kernels too (a run of its own)")
    args = ap.parse_args()
    if args.directed:
        return main_directed(args)
    from cge.jl_amd import api, synth

    ctx = api.Context(0)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        g = synth.abcd_like(s["n"], s["m"], s["C"], s["d"], seed=42)
        ctx.set_graph(g["edges"], g["eweights"], g["n"])
        ctx.set_vertex_data(g["comm"], g["vweights"])
        kw = dict(forced=4, method=s["method"], seed=42, auc_samples=10000)
        for K in [int(k) for k in args.ks.split(",")]:
            embs = embeddings(np.asarray(g["embedding"]), K, seed=K)
            # warm-up and the check: the batch gives what the separate scores give
            got = ctx.score_batch(embs, g["clusters"], s["land"], **kw)
            for e, r in zip(embs, got):
                ctx.set_embedding(e)
                assert np.array_equal(r, ctx.score(g["clusters"], s["land"], **kw)), "batch differs from separate scores"
            seq_ms, seq_sweep, bat_ms, bat_sweep = [], [], [], []
            for _ in range(args.reps):
                t0, sw = time.perf_counter(), 0.0
                for e in embs:
                    ctx.set_embedding(e)
                    ctx.score(g["clusters"], s["land"], **kw)
                    sw += ctx.phase_ms()["sweep"]
                seq_ms.append((time.perf_counter() - t0) * 1e3 / K)
                seq_sweep.append(sw / K)
                t0 = time.perf_counter()
                ctx.score_batch(embs, g["clusters"], s["land"], **kw)
                bat_ms.append((time.perf_counter() - t0) * 1e3 / K)
                bat_sweep.append(ctx.phase_ms()["batch_sweep"] / K)
            n_alpha = [t["n_alpha"] for t in ctx.last_traces]
            print(json.dumps(dict(
                shape=name, K=K, n=g["n"], land=s["land"],
                seq_ms_per_member=round(float(np.median(seq_ms)), 3), batch_ms_per_member=round(float(np.median(bat_ms)), 3),
                seq_sweep_ms_per_member=round(float(np.median(seq_sweep)), 3),
                batch_sweep_ms_per_member=round(float(np.median(bat_sweep)), 3),
                member_alphas=int(sum(n_alpha)), fit_batched_launches=ctx.get_stat("fit_batched_launches"),
                fit_batched_alphas=ctx.get_stat("fit_batched_alphas"),
                launches_per_alpha=round(ctx.get_stat("fit_batched_launches") / max(1, max(n_alpha)), 2),
                reps=args.reps)), flush=True)
    ctx.close()
    return 0


def main_directed(args):
    from cge.jl_amd import api, synth

    def span(v):
        return [round(float(min(v)), 3), round(float(np.median(v)), 3), round(float(max(v)), 3)]

    ctx = api.Context(0)
    if args.fit_timers:
        ctx.profile_enable(True)
        ctx.profile_select(("fit_persistent", "fit_batched"))
    for name in (args.shapes if args.shapes != "n1e4,cfg2" else "n1e4,n1e5").split(","):
        s = DIRECTED_SHAPES[name]
        g = synth.abcd_like(s["n"], s["m"], s["C"], s["d"], seed=42, directed=True)
        ctx.set_graph(g["edges"], g["eweights"], g["n"])
        ctx.set_vertex_data(g["comm"], g["vweights"])
        kw = dict(forced=4, method=s["method"], directed=True, seed=42, auc_samples=10000)
        for K in [int(k) for k in args.ks.split(",")]:
            embs = embeddings(np.asarray(g["embedding"]), K, seed=K)
            got = ctx.score_batch(embs, g["clusters"], s["land"], **kw)  # warm-up and the check
            for e, r in zip(embs, got):
                ctx.set_embedding(e)
                assert np.array_equal(r, ctx.score(g["clusters"], s["land"], **kw)), "batch differs from separate scores"
            seq_ms, seq_sweep, bat_ms, bat_sweep, seq_fit, bat_fit = [], [], [], [], [], []
            for _ in range(args.reps):
                ctx.profile_reset()
                t0, sw = time.perf_counter(), 0.0
                for e in embs:
                    ctx.set_embedding(e)
                    ctx.score(g["clusters"], s["land"], **kw)
                    sw += ctx.phase_ms()["sweep"]
                seq_ms.append((time.perf_counter() - t0) * 1e3 / K)
                seq_sweep.append(sw / K)
                seq_fit.append(ctx.profile().get("fit_persistent", {"total_ms": 0.0})["total_ms"])
                ctx.profile_reset()
                t0 = time.perf_counter()
                ctx.score_batch(embs, g["clusters"], s["land"], **kw)
                bat_ms.append((time.perf_counter() - t0) * 1e3 / K)
                ph = ctx.phase_ms()
                bat_sweep.append((ph.get("batch_sweep", 0.0) + (ph.get("sweep", 0.0) if K == 1 else 0.0)) / K)
                pr = ctx.profile()
                bat_fit.append(sum(pr.get(k, {"total_ms": 0.0})["total_ms"] for k in ("fit_batched", "fit_persistent")))
            n_alpha = [t["n_alpha"] for t in ctx.last_traces]
            print(json.dumps(dict(
                shape=name, directed=True, K=K, n=g["n"], land=s["land"], landmarks=ctx.landmarks_info()[0],
                seq_ms_per_member=span(seq_ms), batch_ms_per_member=span(bat_ms),
                seq_sweep_ms_per_member=span(seq_sweep), batch_sweep_ms_per_member=span(bat_sweep),
                seq_fit_kernel_ms_per_member=span([v / K for v in seq_fit]),
                batch_fit_kernel_ms_per_member=span([v / K for v in bat_fit]),
                member_alphas=int(sum(n_alpha)), fit_iterations=int(sum(sum(t["iters"][:t["n_alpha"]]) for t in ctx.last_traces)),
                fit_batched_launches=ctx.get_stat("fit_batched_launches"), fit_batched_alphas=ctx.get_stat("fit_batched_alphas"),
                reps=args.reps, figures="[min, median, max]")), flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
