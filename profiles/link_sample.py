"""cge_link_sample at the headline shape (synth n = 10^6, m = 10^7, d = 128, -l 4000).

  python profiles/link_sample.py [--scale s] [--draws 3] [--out profiles/link_sample.txt]

  link_fit fits the model of the best local score; then, in the same session: max_pair_kernel on the same operands (the same
  upper tiles, the Gram core alone), `draws` draws with their ids and probabilities fetched -- wall time per call, the kernels'
  own event timers (link_sample, link_sample_sort, link_prob), the pairs evaluated exactly per sampled edge (stat
  "link_sample_survivors"), the edge count against the resident m -- and a count-only call (cap = 0).
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
    ap.add_argument("--draws", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_sample.txt"))
    a = ap.parse_args()
    n, m, C, d, land = int(1_000_000 * a.scale), int(10_500_000 * a.scale), 500, 128, 4000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = synth.abcd_like(n, m, C, d, seed=42)
    ctx = api.Context(0)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    ctx.link_fit(g["clusters"], land, forced=4, method="rss", seed=42, auc_samples=10000)
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
    # ---- the draws
    t0 = time.perf_counter()
    first = ctx.link_sample(1, 0, None, True)  # warm-up: the tables, the scratch (and a second call if 2 m does not hold the set)
    say(f"first call (scratch allocated): {(time.perf_counter() - t0) * 1e3:.1f} ms, {first[3]} edges")
    cap = int(first[3] * 1.1) + 1024
    ctx.profile_reset()
    wall, counts, survs = [], [], []
    for r in range(a.draws):
        t0 = time.perf_counter()
        out = ctx.link_sample(1, r, cap, True)
        wall.append((time.perf_counter() - t0) * 1e3)
        counts.append(out[3])
        survs.append(ctx.get_stat("link_sample_survivors"))
    pr = ctx.profile()
    per = {k: pr[k]["total_ms"] / a.draws for k in ("link_sample", "link_sample_sort", "link_prob") if k in pr}
    assert first[3] == counts[0] and (np.diff(first[0]) >= 0).all()
    say(f"link_sample, {a.draws} draws (streams 0..): wall " + ", ".join(f"{w:.1f}" for w in wall) + " ms; kernels per draw: "
        + ", ".join(f"{k} {v:.2f} ms" for k, v in per.items())
        + f"; link_sample / max_pair_kernel = {per['link_sample'] / mp_ms:.2f} ({ctx.get_stat('link_sample_tiles')} tiles)")
    say("edges per draw: " + ", ".join(str(c) for c in counts) + f" against the resident m = {m_res} ({np.mean(counts) / m_res:.3f} m); "
        "evaluated exactly: " + ", ".join(str(s) for s in survs) + f" = {np.sum(survs) / np.sum(counts):.4f} per sampled edge")
    ctx.profile_reset()
    t0 = time.perf_counter()
    ne = ctx.link_sample(1, 0, 0)[3]
    say(f"count only (cap = 0): wall {(time.perf_counter() - t0) * 1e3:.1f} ms, kernel {ctx.profile()['link_sample']['total_ms']:.2f} ms, "
        f"{ne} edges")
    deg = np.bincount(np.concatenate([first[0], first[1]]) - 1, minlength=g["n"])
    e = np.asarray(g["edges"])
    deg0 = np.bincount(np.concatenate([e[:, 0], e[:, 1]]) - 1, minlength=g["n"])
    say(f"degrees: the sample's mean {deg.mean():.2f} / max {deg.max()}, the graph's {deg0.mean():.2f} / {deg0.max()}; "
        f"correlation {np.corrcoef(deg, deg0)[0, 1]:.4f}")
    open(a.out, "w").write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
