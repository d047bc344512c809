"""The link model's calls at the headline shape (synth n = 10^6, m = 10^7, d = 128, -l 4000).

  python profiles/link_topk.py [--scale s] [--out profiles/link_topk.txt]

  link_topk   k = 32, Q in {1024, 16384}: wall time per call, min / median / max of 5 calls after a warm-up, the kernels' own event
              timers, and the survivors per query (pairs the filter let through; stat "link_topk_survivors").  The time is set
              against 2 Q n dpad flop at the fp64 rate max_pair_kernel reaches on the same operands in the same session (its
              timer and its tile count): the same tile core with the cheapest possible epilogue.
  link_prob   10^6 random pairs, beside pair_dist's timer of the score's own sampled pairs.
  link_fit    against cge_score on the same context, alternated, 10 calls a side: the difference is the copy and the expansion.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cge.jl_amd import api, synth  # noqa: E402


def stats(v):
    v = sorted(v)
    return f"min {v[0]:.3f} / median {v[len(v) // 2]:.3f} / max {v[-1]:.3f} ms"


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_topk.txt"))
    a = ap.parse_args()
    n, m, C, d, land = int(1_000_000 * a.scale), int(10_500_000 * a.scale), 500, 128, 4000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = synth.abcd_like(n, m, C, d, seed=42)
    ctx = api.Context(0)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    kw = dict(forced=4, method="rss", seed=42, auc_samples=10000)
    say(f"graph: n = {g['n']}, m = {g['m']}, d = {d}, -l {land}")
    # ---- link_fit against cge_score, alternated
    ctx.score(g["clusters"], land, **kw)
    ctx.link_fit(g["clusters"], land, **kw)
    ts, tf = [], []
    for _ in range(10):
        ts += timed(lambda: ctx.score(g["clusters"], land, **kw), 1)
        tf += timed(lambda: ctx.link_fit(g["clusters"], land, **kw), 1)
    vec, _ = ctx.link_fit(g["clusters"], land, **kw)
    assert vec.tobytes() == ctx.score(g["clusters"], land, **kw).tobytes()
    ctx.link_fit(g["clusters"], land, **kw)
    mdl = ctx.link_model()
    say(f"cge_score : {stats(ts)}")
    say(f"link_fit  : {stats(tf)}   (model: alpha {mdl['alpha']}, hi {mdl['hi']:.6g}, f in [{mdl['f_out'].min():.3g}, {mdl['f_out'].max():.3g}])")
    # ---- the rate of the tile core: max_pair_kernel on the same operands
    dpad, nT = (d + 15) // 16 * 16, (g["n"] + 127) // 128
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.max_pair_dist()
    mp = ctx.profile()["max_pair_dist"]
    mp_flop = nT * (nT + 1) / 2 * 2.0 * 128 * 128 * dpad
    rate = mp_flop / (mp["total_ms"] / mp["launches"] * 1e-3)
    say(f"max_pair_kernel: {mp['total_ms'] / mp['launches']:.2f} ms for {nT * (nT + 1) // 2} tiles = {rate / 1e12:.2f} Tflop/s (fp64)")
    # ---- link_topk
    rng = np.random.default_rng(1)
    for Q in (1024, 16384):
        q = rng.integers(1, g["n"] + 1, Q)
        ctx.link_topk(q, 32, True)  # warm-up (the edge keys, the scratch)
        ctx.profile_reset()
        wall = timed(lambda: ctx.link_topk(q, 32, True), 5)
        pr = ctx.profile()
        kern = pr["link_topk"]["total_ms"] / pr["link_topk"]["launches"]
        merge = pr["link_merge"]["total_ms"] / pr["link_merge"]["launches"]
        ideal = 2.0 * Q * g["n"] * dpad / rate * 1e3
        surv = ctx.get_stat("link_topk_survivors") / Q
        say(f"link_topk Q = {Q}, k = 32: wall {stats(wall)}; kernel {kern:.3f} ms + merge {merge:.3f} ms; "
            f"2 Q n dpad flop at max_pair_kernel's rate = {ideal:.3f} ms; ratio {kern / ideal:.2f}; survivors per query {surv:.0f}")
    # ---- link_prob
    i, j = rng.integers(1, g["n"] + 1, 1_000_000), rng.integers(1, g["n"] + 1, 1_000_000)
    ctx.link_prob(i, j)
    ctx.profile_reset()
    wall = timed(lambda: ctx.link_prob(i, j), 5)
    pr = ctx.profile()
    say(f"link_prob 10^6 pairs: wall {stats(wall)}; kernel {pr['link_prob']['total_ms'] / pr['link_prob']['launches']:.3f} ms")
    ctx.profile_reset()
    ctx.score(g["clusters"], land, **kw)
    pr = ctx.profile()
    if "pair_dist" in pr and pr["pair_dist"]["launches"]:
        say(f"pair_dist of one score (2 x 10^4 sampled pairs): {pr['pair_dist']['total_ms'] / pr['pair_dist']['launches']:.3f} ms per launch")
    open(a.out, "w").write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
