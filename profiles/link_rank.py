"""cge_link_rank at the headline shape (synth n = 10^6, m = 10^7, d = 128, -l 4000).

  python profiles/link_rank.py [--scale s] [--held-out 10000] [--out profiles/link_rank.txt]

  10 000 random edges are held out, link_fit runs on the rest, link_rank ranks the held-out edges with exclusion on: wall time
  per call (min / median / max of 5 calls after a warm-up), the kernels' own event timers, survivors per pair and per distinct
  query (stat "link_rank_survivors"), the median `greater`, api.link_metrics.  The counting kernel's time is set against
  2 Qu n dpad flop at the fp64 rate max_pair_kernel reaches on the same operands in the same session, as profiles/link_topk.py
  does for top-k.
  Brute force, what a user had before: one link_prob call over all n candidates of a query -- wall time and ids uploaded,
  measured for 16 queries (whose counts are compared with link_rank's) and scaled to the distinct queries.
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
    ap.add_argument("--held-out", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_rank.txt"))
    a = ap.parse_args()
    n, m, C, d, land = int(1_000_000 * a.scale), int(10_500_000 * a.scale), 500, 128, 4000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = synth.abcd_like(n, m, C, d, seed=42)
    e = np.asarray(g["edges"])
    rng = np.random.default_rng(1)
    rows = rng.choice(len(e), a.held_out, replace=False)
    rows = rows[e[rows, 0] != e[rows, 1]]
    keep = np.ones(len(e), bool)
    keep[rows] = False
    test = e[rows]
    ctx = api.Context(0)
    ctx.set_inputs(np.asfortranarray(e[keep]), np.asarray(g["eweights"])[keep], g["vweights"], g["comm"], g["embedding"])
    kw = dict(forced=4, method="rss", seed=42, auc_samples=10000)
    ctx.link_fit(g["clusters"], land, **kw)
    mdl = ctx.link_model()
    say(f"graph: n = {g['n']}, m = {int(keep.sum())} training edges + {len(test)} held out, d = {d}, -l {land}; "
        f"model: alpha {mdl['alpha']}, hi {mdl['hi']:.6g}")
    # ---- the rate of the tile core: max_pair_kernel on the same operands
    dpad, nT = (d + 15) // 16 * 16, (g["n"] + 127) // 128
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.max_pair_dist()
    mp = ctx.profile()["max_pair_dist"]
    rate = nT * (nT + 1) / 2 * 2.0 * 128 * 128 * dpad / (mp["total_ms"] / mp["launches"] * 1e-3)
    say(f"max_pair_kernel: {mp['total_ms'] / mp['launches']:.2f} ms = {rate / 1e12:.2f} Tflop/s (fp64)")
    # ---- link_rank
    i, j = test[:, 0], test[:, 1]
    P = len(i)
    gr, ti, cand, p = ctx.link_rank(i, j, True)  # warm-up (the edge keys, the excluded counts, the scratch)
    ctx.profile_reset()
    wall = timed(lambda: ctx.link_rank(i, j, True), 5)
    pr = ctx.profile()
    per = {k: pr[k]["total_ms"] / 5 for k in ("link_rank", "link_rank_final", "link_prob") if k in pr}
    Qu, surv = ctx.get_stat("link_rank_queries"), ctx.get_stat("link_rank_survivors")
    ideal = 2.0 * Qu * g["n"] * dpad / rate * 1e3
    say(f"link_rank P = {P} pairs of {Qu} distinct queries: wall {stats(wall)}; kernels per call: "
        + ", ".join(f"{k} {v:.3f} ms" for k, v in per.items())
        + f"; 2 Qu n dpad flop at max_pair_kernel's rate = {ideal:.3f} ms; ratio {per['link_rank'] / ideal:.2f}")
    say(f"survivors: {surv} = {surv / P:.0f} per pair, {surv / Qu:.0f} per distinct query ({100.0 * surv / (Qu * g['n']):.2f} % of the "
        f"candidates); median greater {int(np.median(gr))}, pairs with ties {int((ti > 0).sum())}, median cand {int(np.median(cand))}")
    say("metrics: " + " ".join(f"{k}={v:.6g}" for k, v in api.link_metrics(gr, ti, cand).items()))
    # ---- brute force: every candidate of a query through link_prob
    allc = np.arange(1, g["n"] + 1, dtype=np.int64)
    qs = np.unique(i)[:16]
    ctx.link_prob(np.full(g["n"], qs[0]), allc)
    tb, tr = [], e[keep]
    for q in qs:
        t0 = time.perf_counter()
        vals = ctx.link_prob(np.full(g["n"], q), allc)
        tb.append((time.perf_counter() - t0) * 1e3)
        for s in np.flatnonzero(i == q):  # (the comparison is outside the user's cost only by the exclusion, done here in numpy)
            ok = np.ones(g["n"], bool)
            ok[[q - 1, j[s] - 1]] = False
            ok[tr[tr[:, 0] == q, 1] - 1] = False
            ok[tr[tr[:, 1] == q, 0] - 1] = False
            assert (int((vals[ok] > p[s]).sum()), int((vals[ok] == p[s]).sum()), int(ok.sum())) == (gr[s], ti[s], cand[s]), (q, s)
    per_q = float(np.median(tb))
    say(f"brute force: link_prob over all n candidates of one query: wall {stats(tb)} ({16 * g['n'] / 1e6:.0f} MB of ids uploaded per "
        f"query); x {Qu} distinct queries = {per_q * Qu / 1e3:.1f} s against link_rank's {sorted(wall)[2] / 1e3:.3f} s: "
        f"{per_q * Qu / sorted(wall)[2]:.0f} times; the 16 queries' counts agree with link_rank's")
    open(a.out, "w").write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
