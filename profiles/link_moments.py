"""cge_link_moments on a fitted model: synth n = 10^5, m = 10^6, d = 128, -l 4000 by default.

  python profiles/link_moments.py [--scale s] [--calls 2] [--out profiles/link_moments.txt]

  link_fit fits the model of the best divergence; then, in the same session: max_pair_kernel on the same operands' upper tiles
  (the Gram core alone), `calls` whole calls of cge_link_moments -- wall time per call, the kernels' own event timers
  (link_moments, link_moments_final), the four stats, the scratch bytes by the formula of link_host.cpp -- and global_vertex
  (the JS divergence of the observed bins against the model summed over all vertex pairs) beside element 2 of the score.
  --scale 10 is the headline graph; --calls 0 measures the first call and makes no other.  --test115 adds the same two figures
  for tests/golden/test115 (-l 20 and -l 40).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cge.jl_amd import api, synth  # noqa: E402


def scratch_bytes(n, d, comm, directed):
    """link_host.cpp's formula: 8 dpad ldn + 16 wb 128 items + 64 slots + 16 L + 32 n."""
    dpad, nT = (d + 15) // 16 * 16, (n + 127) // 128
    wb = 2
    while (nT + wb - 1) // wb > 512:
        wb *= 2
    nB, bs = (nT + wb - 1) // wb, wb * 128
    cs = np.sort(np.asarray(comm, np.int64).ravel())
    rank = np.cumsum(np.r_[0, np.diff(cs) > 0])
    nc = np.array([rank[min(n - 1, (S + 1) * bs - 1)] - rank[S * bs] + 1 for S in range(nB)], np.int64)
    C = int(cs.max())
    if directed:
        items, slots, L = nB * nB, int(nc.sum()) ** 2, C * C
    else:
        items, L = nB * (nB + 1) // 2, C * (C + 1) // 2
        suffix = np.cumsum(nc[::-1])[::-1]
        slots = int((nc * suffix).sum())
    return 8 * dpad * nT * 128 + 16 * wb * 128 * items + 64 * slots + 16 * L + 32 * n, wb, items, slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--test115", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_moments.txt"))
    a = ap.parse_args()
    n, m, C, d, land = int(100_000 * a.scale), int(1_050_000 * a.scale), max(50, int(50 * a.scale)), 128, 4000
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        open(a.out, "a").write(s + "\n")

    if a.test115:
        from cge.jl_amd import parseargs

        gd = os.path.join(ROOT, "tests", "golden", "test115")
        keys = ("edges", "eweights", "vweights", "comm", "clusters", "embedding")
        g = dict(zip(keys, parseargs(["-g", f"{gd}/test.edgelist", "-c", f"{gd}/test1col.ecg", "-e", f"{gd}/test_n2v.embedding", "-l", "20"],
                                     exit_on_error=False)))
        ctx = api.Context(0)
        ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
        for land115 in (20, 40, -1):
            vec, _ = ctx.link_fit(g["clusters"], land115, forced=4, method="rss", seed=17, auc_samples=500, which="global")
            mo = ctx.link_moments(land115 == -1)
            gv = api.link_divergence(mo.C, mo.B, mo.n_comm, False, False, ctx=ctx)["global"]
            say(f"test115 -l {land115} ({len(ctx.link_model()['T_out'])} iterates): alpha {vec[0]}, global_sweep {vec[1]:.9f}, "
                f"global_vertex {gv:.9f}{' (diag = 1)' if land115 == -1 else ''}")
        ctx.close()
        return
    g = synth.abcd_like(n, m, C, d, seed=42)
    ctx = api.Context(0)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    vec, _ = ctx.link_fit(g["clusters"], land, forced=4, method="rss", seed=42, auc_samples=10000, which="global")
    mdl = ctx.link_model()
    ff = np.sort(mdl["f_out"])
    say(f"graph: n = {g['n']}, m = {len(g['eweights'])}, d = {d}, C = {int(np.asarray(g['comm']).max())}, -l {land}; model: alpha "
        f"{mdl['alpha']}, hi {mdl['hi']:.6g}, f in [{ff[0]:.3g}, {ff[-1]:.3g}], median {ff[len(ff) // 2]:.3g}")
    dpad, nT = (d + 15) // 16 * 16, (g["n"] + 127) // 128
    sb, wb, items, slots = scratch_bytes(g["n"], d, g["comm"], False)
    say(f"scratch: {sb} bytes = {sb / 2 ** 30:.3f} GiB (wb {wb}, {items} work items, {slots} bin slots)")
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.max_pair_dist()
    mp = ctx.profile()["max_pair_dist"]
    mp_ms = mp["total_ms"] / mp["launches"]
    say(f"max_pair_kernel: {mp_ms:.2f} ms over {nT * (nT + 1) // 2} tiles = "
        f"{nT * (nT + 1) / 2 * 2.0 * 128 * 128 * dpad / (mp_ms * 1e-3) / 1e12:.2f} Tflop/s (fp64)")
    keys = ("link_moments", "link_moments_final")
    ctx.profile_reset()
    t0 = time.perf_counter()
    first = mo = ctx.link_moments()
    wall = [(time.perf_counter() - t0) * 1e3]
    say(f"first call (scratch allocated): {wall[0]:.1f} ms")
    if a.calls > 0:
        ctx.profile_reset()
        wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        mo = ctx.link_moments()
        wall.append((time.perf_counter() - t0) * 1e3)
    pr = ctx.profile()
    st = {k: ctx.get_stat("link_moments_" + k) for k in ("exact", "fast", "saturated", "tiles")}
    per = {k: pr[k]["total_ms"] / max(a.calls, 1) for k in keys if k in pr}
    assert np.array_equal(mo.B, first.B) and np.array_equal(mo.deg_out, first.deg_out)
    pairs = g["n"] * (g["n"] - 1) // 2
    ratio = per["link_moments"] / mp_ms
    say(f"link_moments, {max(a.calls, 1)} call(s): wall " + ", ".join(f"{w:.1f}" for w in wall) + " ms; kernels per call: "
        + ", ".join(f"{k} {v:.2f} ms" for k, v in per.items())
        + f"; link_moments / max_pair_kernel = {ratio:.2f} (the epilogue's share, taking max_pair_kernel for the Gram core: "
        f"{1 - 1 / ratio:.2f}); {per['link_moments'] * 1e6 / pairs:.4f} ns per pair")
    say(f"stats: {st} of {pairs} pairs")
    gv = api.link_divergence(mo.C, mo.B, mo.n_comm, False, False, ctx=ctx)["global"]
    vw = np.asarray(g["vweights"], np.float64).ravel()
    rel = np.abs(mo.deg_out - vw) / np.maximum(vw, 1.0)
    say(f"global_vertex {gv:.9f}, global_sweep (element 2) {vec[1]:.9f}, alpha {vec[0]}; expected edges {mo.B.sum():.1f} of "
        f"{len(g['eweights'])}; |expected degree - weight| / max(weight, 1): median {np.median(rel):.3f}, 99th percentile "
        f"{np.percentile(rel, 99):.3f}")
    ctx.close()


if __name__ == "__main__":
    main()
