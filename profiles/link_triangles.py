"""cge_link_triangles on a fitted model: synth.abcd_like(n, 10 n, ...), d = 128, -l 4000, the model of
the best local score.

  python profiles/link_triangles.py --n 20000 [--calls 2] [--out profiles/link_triangles.txt]
  python profiles/link_triangles.py --largest        the largest n whose Q fits in 85% of the free device memory
  python profiles/link_triangles.py --test115        tests/golden/test115, -l 20 / 40 / exact

  In one session: max_pair_kernel on the headline operands (the Gram core alone, the floor in Tflop/s), then the first call of
  cge_link_triangles (Q allocated) and `calls` more -- wall time per call and the kernels' own event timers: link_tri_q (the
  generator), link_tri (the triangle kernel; its flops are 2 * 128 nT * 128^2 * tiles), link_tri_final, link_wedge,
  link_tri_observed (keys to counts) -- and what the library now tells: transitivity observed against expected.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cge.jl_amd import api, synth  # noqa: E402

KEYS = ("link_tri_q", "link_tri", "link_tri_final", "link_wedge", "link_tri_observed")


def gram_floor(ctx, say):
    """max_pair_kernel on the headline operands (n = 10^5, d = 128): Tflop/s of the Gram core."""
    g = synth.abcd_like(100_000, 1_050_000, 50, 128, seed=42)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    ctx.profile_enable(True)
    ctx.max_pair_dist()
    ctx.profile_reset()
    ctx.max_pair_dist()
    mp = ctx.profile()["max_pair_dist"]
    ms = mp["total_ms"] / mp["launches"]
    nT = (100_000 + 127) // 128
    tf = nT * (nT + 1) / 2 * 2.0 * 128 * 128 * 128 / (ms * 1e-3) / 1e12
    say(f"max_pair_kernel, n = 100000, d = 128: {ms:.2f} ms over {nT * (nT + 1) // 2} tiles = {tf:.2f} Tflop/s (fp64)")
    return tf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--largest", action="store_true")
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--test115", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "link_triangles.txt"))
    a = ap.parse_args()

    def say(s):
        print(s, flush=True)
        open(a.out, "a").write(s + "\n")

    if a.test115:
        from cge.jl_amd import parseargs

        gd = os.path.join(ROOT, "tests", "golden", "test115")
        keys = ("edges", "eweights", "vweights", "comm", "clusters", "embedding")
        g = dict(zip(keys, parseargs(["-g", f"{gd}/test.edgelist", "-c", f"{gd}/test1col.ecg", "-e", f"{gd}/test_n2v.embedding", "-l", "20"],
                                     exit_on_error=False)))
        ctx = api.Context(0)
        ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
        for land in (20, 40, -1):
            vec, _ = ctx.link_fit(g["clusters"], land, forced=4, method="rss", seed=17, auc_samples=2000, which="local")
            t = api.link_clustering_table(*ctx.link_triangles())
            say(f"test115 -l {land}: alpha {vec[0]}, transitivity observed {t['transitivity_obs']:.4f} expected {t['transitivity_exp']:.4f}; "
                f"triangles observed {t['triangles_obs']:.0f} expected {t['triangles_exp']:.1f}")
        ctx.close()
        return
    ctx = api.Context(0)
    tf_floor = gram_floor(ctx, say)
    n = a.n
    if a.largest:
        import ctypes

        fr, tot = ctypes.c_size_t(), ctypes.c_size_t()
        assert ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(fr), ctypes.byref(tot)) == 0
        free = fr.value
        n = (int(np.sqrt(0.85 * free / 8)) // 128 - 1) * 128
        say(f"largest: {free} bytes free, n = {n}")
    g = synth.abcd_like(n, 10 * n, max(50, n // 2000), 128, seed=42)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    vec, _ = ctx.link_fit(g["clusters"], 4000, forced=4, method="rss", seed=42, auc_samples=10000, which="local")
    mdl = ctx.link_model()
    nT = (n + 127) // 128
    ld, tiles = 128 * (nT | 1), nT * (nT + 1) // 2
    say(f"graph: n = {n}, m = {len(g['eweights'])}, d = 128, -l 4000; model: alpha {mdl['alpha']}, hi {mdl['hi']:.6g}; ld = {ld}, Q = "
        f"{8 * ld * ld / 2 ** 30:.2f} GiB, partials {8 * 128 * nT * nT / 2 ** 30:.3f} GiB, {tiles} tiles")
    ctx.profile_reset()
    t0 = time.perf_counter()
    first = res = ctx.link_triangles()
    wall = [(time.perf_counter() - t0) * 1e3]
    say(f"first call (Q allocated): {wall[0]:.1f} ms")
    if a.calls > 0:
        ctx.profile_reset()
        wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        res = ctx.link_triangles()
        wall.append((time.perf_counter() - t0) * 1e3)
    for x, y in zip(res, first):
        assert np.array_equal(x, y)
    pr = ctx.profile()
    per = {k: pr[k]["total_ms"] / max(a.calls, 1) for k in KEYS if k in pr}
    flops = 2.0 * 128 * nT * 128 * 128 * tiles
    tf = flops / (per["link_tri"] * 1e-3) / 1e12
    say(f"link_triangles, {max(a.calls, 1)} call(s): wall " + ", ".join(f"{w:.1f}" for w in wall) + " ms; kernels per call: "
        + ", ".join(f"{k} {v:.2f} ms" for k, v in per.items()))
    say(f"link_tri: {flops:.4g} flop = {tf:.2f} Tflop/s; Gram floor / link_tri = {tf_floor / tf:.2f}; saturated pairs "
        f"{ctx.get_stat('link_tri_saturated')}")
    t = api.link_clustering_table(*res)
    say(f"transitivity observed {t['transitivity_obs']:.5f} expected {t['transitivity_exp']:.5f}; triangles observed "
        f"{t['triangles_obs']:.0f} expected {t['triangles_exp']:.1f}; wedges observed {t['summary'][3]:.0f} expected {t['summary'][1]:.1f}")
    ctx.close()


if __name__ == "__main__":
    main()
