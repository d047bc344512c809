"""cge_link_auc on a fitted model: synth n = 10^5, m = 10^6, d = 128, -l 4000 by default.

  python profiles/link_auc.py [--scale s] [--calls 2] [--part-of P] [--out profiles/link_auc.txt]

  link_fit fits the model of the best local score; then, in the same session: max_pair_kernel on the same operands (the same
  upper tiles, the Gram core alone), `calls` whole calls of cge_link_auc -- wall time per call, the kernels' own event timers
  (link_prob, link_auc_sort, link_auc, link_auc_final), the three stats, the exact local score beside the sampled one -- and,
  with --part-of P, ONE call of part 0 of P alone (what a graph too large for one call is measured by).  --scale 10 is the
  headline graph; --calls 0 measures the first call and makes no other.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cge.jl_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--part-of", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_auc.txt"))
    a = ap.parse_args()
    n, m, C, d, land = int(100_000 * a.scale), int(1_050_000 * a.scale), max(50, int(50 * a.scale)), 128, 4000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        open(a.out, "w").write("\n".join(lines) + "\n")

    g = synth.abcd_like(n, m, C, d, seed=42)
    ctx = api.Context(0)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    vec, _ = ctx.link_fit(g["clusters"], land, forced=4, method="rss", seed=42, auc_samples=10000)
    mdl = ctx.link_model()
    m_res = len(g["eweights"])
    ff = np.sort(mdl["f_out"])
    say(f"graph: n = {g['n']}, m = {m_res}, d = {d}, -l {land}; model: alpha {mdl['alpha']}, hi {mdl['hi']:.6g}, "
        f"f in [{ff[0]:.3g}, {ff[-1]:.3g}], median {ff[len(ff) // 2]:.3g}")
    dpad, nT = (d + 15) // 16 * 16, (g["n"] + 127) // 128
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.max_pair_dist()
    mp = ctx.profile()["max_pair_dist"]
    mp_ms = mp["total_ms"] / mp["launches"]
    say(f"max_pair_kernel: {mp_ms:.2f} ms over {nT * (nT + 1) // 2} tiles = "
        f"{nT * (nT + 1) / 2 * 2.0 * 128 * 128 * dpad / (mp_ms * 1e-3) / 1e12:.2f} Tflop/s (fp64)")
    keys = ("link_prob", "link_auc_sort", "link_auc", "link_auc_final")

    def stats():
        return {k: ctx.get_stat("link_auc_" + k) for k in ("survivors", "proven", "tiles")}

    if a.part_of > 1:
        ctx.profile_reset()
        t0 = time.perf_counter()
        r = ctx.link_auc(0, a.part_of)
        wall = (time.perf_counter() - t0) * 1e3
        pr, st = ctx.profile(), stats()
        say(f"link_auc part 0 of {a.part_of} (first call, scratch allocated): wall {wall:.1f} ms; kernels: "
            + ", ".join(f"{k} {pr[k]['total_ms']:.2f} ms" for k in keys if k in pr)
            + f"; {st}; link_auc x {a.part_of} / max_pair_kernel = {pr['link_auc']['total_ms'] * a.part_of / mp_ms:.2f}; "
            f"{pr['link_auc']['total_ms'] * 1e6 / max(st['survivors'], 1):.3f} ns per pair evaluated; n_neg {r['n_neg']}")
    else:
        ctx.profile_reset()
        t0 = time.perf_counter()
        first = r = ctx.link_auc(want_counts=True)
        wall = [(time.perf_counter() - t0) * 1e3]
        say(f"first call (scratch allocated): {wall[0]:.1f} ms")
        if a.calls > 0:  # (--calls 0: the first call is the measurement -- the headline graph, minutes a call)
            ctx.profile_reset()
            wall = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            r = ctx.link_auc(want_counts=True)
            wall.append((time.perf_counter() - t0) * 1e3)
        pr, st = ctx.profile(), stats()
        per = {k: pr[k]["total_ms"] / max(a.calls, 1) for k in keys if k in pr}
        assert r["L"] == first["L"] and r["Tq"] == first["Tq"]
        pairs = g["n"] * (g["n"] - 1) // 2
        say(f"link_auc, {max(a.calls, 1)} call(s): wall " + ", ".join(f"{w:.1f}" for w in wall) + " ms; kernels per call: "
            + ", ".join(f"{k} {v:.2f} ms" for k, v in per.items())
            + f"; link_auc / max_pair_kernel = {per['link_auc'] / mp_ms:.2f}")
        say(f"stats: {st} of {pairs} pairs ({st['survivors'] / pairs:.4f} evaluated exactly, "
            f"{per['link_auc'] * 1e6 / max(st['survivors'], 1):.3f} ns each); n_neg {r['n_neg']}, rows with ties {int((r['ties'] > 0).sum())}")
        sd = np.sqrt(r["local_exact"] * (1 - r["local_exact"]) / 10000)
        say(f"local score: exact {r['local_exact']:.9f}, AUC {r['auc']:.9f}; sampled (element 6, 10000 samples) {vec[5]:.6f} "
            f"+- {vec[6]:.6f} = {(vec[5] - r['local_exact']) / sd:+.2f} sd from the exact value")
    ctx.close()


if __name__ == "__main__":
    main()
