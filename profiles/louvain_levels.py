"""The Louvain hierarchy on the headline graph's generator: what each level looks like and what it costs.

    python profiles/louvain_levels.py [--n 1000000] [--m 10000000] [--parent-lib FILE] [--reps 10]

Per level: vertices, adjacency entries, longest segment (from the numpy contraction of the original list by the level before),
communities, rounds; the contraction's and the pass's time (event pairs, `louvain_contract_L<k>` / `louvain_pass_L<k>`) with the
lane form alone and with the wave form from a few segment lengths on (testing knob `louvain_wave_len`).  All runs must return
the same levels (unit weights: exact).

--parent-lib: the level-1 regression guard.  Two worker processes, one per build of the library, each with the graph resident;
`cge_louvain` is timed in turn, one call a side, `reps` times.  The rule: this build stays under the parent's
slowest repetition plus the parent's own spread."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LANE_ONLY = 2**31 - 1


def worker(lib, graph_file):
    from cge.jl_amd import api

    if lib != "-":
        api._LIB_PATH = os.path.abspath(lib)
    e = np.load(graph_file)
    ctx = api.Context(0)
    ctx.set_graph(e, np.ones(len(e)), int(e.max()))
    ctx.louvain()  # warm-up
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "run":
            break
        t0 = time.perf_counter()
        _, nc, q, rounds = ctx.louvain()
        print(f"{(time.perf_counter() - t0) * 1e3:.3f} {nc} {q!r} {rounds}", flush=True)
    ctx.close()


def level_shapes(e0, n, levels):
    """(vertices, adjacency entries, longest segment) of every level's own graph."""
    shapes, comp, nn = [], np.arange(n), n
    for comm, nc, _, _ in levels:
        cu, cv = comp[e0[:, 0]], comp[e0[:, 1]]
        keep = cu != cv
        pairs = np.unique(np.minimum(cu[keep], cv[keep]) * nn + np.maximum(cu[keep], cv[keep]))
        deg = np.bincount(np.concatenate([pairs // nn, pairs % nn]), minlength=nn)
        if nn == n:  # level 1 keeps repeated edges as separate entries
            deg = np.bincount(np.concatenate([cu[keep], cv[keep]]), minlength=nn)
        shapes.append((nn, int(deg.sum()), int(deg.max())))
        comp, nn = comm, nc
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10**6)
    ap.add_argument("--m", type=int, default=10**7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--worker", nargs=2, default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    from cge.jl_amd import api, synth

    t0 = time.time()
    g = synth.abcd_like(a.n, a.m, 500, 2, seed=42)  # (d = 2: only the graph is used)
    e = np.ascontiguousarray(g["edges"])
    n = g["n"]
    print(f"graph: n {n}, m {len(e)}, planted communities 500 ({time.time() - t0:.1f} s)", flush=True)
    ctx = api.Context(0)
    ctx.set_graph(e, np.ones(len(e)), n)
    ctx.louvain_levels()  # warm-up
    ctx.profile_enable(True)
    base = None
    for knob in (LANE_ONLY, 1024, 256, 128, 64, 32, -1):
        ctx.set_option("louvain_wave_len", knob)
        best = None
        for _ in range(3):
            ctx.profile_reset()
            t0 = time.perf_counter()
            lv = ctx.louvain_levels()
            wall = (time.perf_counter() - t0) * 1e3
            prof = ctx.profile()
            if best is None or wall < best[0]:
                best = (wall, prof)
        if base is None:
            base = lv
            shapes = level_shapes(e - 1, n, lv)
            for l, ((_, nc, q, r), (nn, ent, longest)) in enumerate(zip(lv, shapes)):
                print(f"level {l + 1}: vertices {nn}, adjacency entries {ent}, longest segment {longest} -> communities {nc}, "
                      f"modularity {q:.6f}, rounds {r}", flush=True)
        else:
            assert len(lv) == len(base) and all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(lv, base)), knob
        name = {LANE_ONLY: "lane form only", -1: "wave form, every vertex"}.get(knob, f"wave form from {knob} entries")
        wall, prof = best
        row = []
        for l in range(1, len(lv) + 2):
            p_ms = prof.get(f"louvain_pass_L{l}", {}).get("total_ms")
            c_ms = prof.get(f"louvain_contract_L{l}", {}).get("total_ms")
            if p_ms is not None:
                row.append(f"L{l} " + (f"contract {c_ms:.2f} + " if c_ms is not None else "") + f"pass {p_ms:.2f}")
        print(f"{name:28s} whole call {wall:8.2f} ms | " + " | ".join(row), flush=True)
    ctx.set_option("louvain_wave_len", -2)
    ctx.profile_enable(False)
    ctx.close()
    if not a.parent_lib:
        return
    import tempfile

    out_dir = tempfile.mkdtemp()
    graph_file = os.path.join(out_dir, "louvain_levels_graph.npy")
    np.save(graph_file, e)
    sides = {}
    try:
        for side, lib in (("parent", a.parent_lib), ("this", "-")):
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib, graph_file], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True)
            assert p.stdout.readline().strip() == "ready", side
            sides[side] = (p, [])
        for _ in range(a.reps):
            for side in ("parent", "this"):
                p, ms = sides[side]
                p.stdin.write("run\n")
                p.stdin.flush()
                ms.append(p.stdout.readline().split())
    finally:
        for p, _ in sides.values():
            p.stdin.close()
            p.wait(timeout=120)
        os.remove(graph_file)
        os.rmdir(out_dir)
    assert all(r[1:] == sides["parent"][1][0][1:] for _, rs in sides.values() for r in rs), "the two builds disagree"
    t = {side: np.array([float(r[0]) for r in rs]) for side, (_, rs) in sides.items()}
    for side in ("parent", "this"):
        print(f"cge_louvain, {side:6s} build: min {t[side].min():.2f} median {np.median(t[side]):.2f} max {t[side].max():.2f} ms "
              f"({a.reps} calls, in turn)")
    bound = t["parent"].max() + (t["parent"].max() - t["parent"].min())
    print(f"rule: this build's median {np.median(t['this']):.2f} ms and slowest {t['this'].max():.2f} ms against the parent's slowest + "
          f"spread {bound:.2f} ms: {'within' if t['this'].max() <= bound else 'median within' if np.median(t['this']) <= bound else 'OVER'}")


if __name__ == "__main__":
    main()
