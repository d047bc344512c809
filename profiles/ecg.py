"""ECG (`cge_ecg`) on the headline graph's generator: what it finds and what it costs.

    python profiles/ecg.py [--sizes 10000,100000,1000000] [--reps 5] [--groups 1,2,4,8,16] [--parent-lib FILE]

Per size n (synth.abcd_like(n, 10 n, C) with C = 50 / 160 / 500 planted communities; K = 16 members, w_min = 0.05):

* quality: ARI against the planted communities and the number of communities for Louvain's level 1, its last level and ECG;
* the whole call (host clock around `Context.ecg`, which ends in a synchronise) with the members in lock-step groups of g for
  every g of --groups, in alternation: one call per g, then the next repetition -- min / median / max of `reps` after a warm-up
  of every g.  g = 1 is one member at a time.  Every g must return the same members, bit for bit (unit weights; the final
  partition is on real weights, where two calls may break a tie differently, so it is printed, not compared);
* the stages of the call (event pairs around each stage: ranks, members, peel, weights, hierarchy, modularity), median of `reps`,
  at the default group size and at g = 1.

--parent-lib: the guard for the kernels the members share with `cge_louvain` (the workers of profiles/louvain_levels.py: two
processes, one per build, the n = 10^6 graph resident, one call a side in turn, 10 times; DESIGN 4.7's rule)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PLANTED = {10**4: 50, 10**5: 160, 10**6: 500}
STAGES = ("ecg_ranks", "ecg_members", "ecg_peel", "ecg_weights", "ecg_hierarchy", "ecg_modularity")
K, W_MIN, SEED = 16, 0.05, 0


def ari(a, b):
    """Adjusted Rand index from the non-empty cells of the contingency table."""
    a, b = np.unique(a, return_inverse=True)[1].astype(np.int64), np.unique(b, return_inverse=True)[1].astype(np.int64)
    c2 = lambda x: (x * (x - 1.0) / 2.0).sum()
    cells = np.unique(a * (b.max() + 1) + b, return_counts=True)[1].astype(np.float64)
    s, sa, sb, tot = c2(cells), c2(np.bincount(a).astype(np.float64)), c2(np.bincount(b).astype(np.float64)), len(a) * (len(a) - 1.0) / 2.0
    exp = sa * sb / tot
    return float((s - exp) / (0.5 * (sa + sb) - exp))


def spread(ms):
    return f"min {min(ms):9.2f} median {np.median(ms):9.2f} max {max(ms):9.2f} ms"


def one_size(api, synth, n, reps, groups):
    t0 = time.time()
    g = synth.abcd_like(n, 10 * n, PLANTED.get(n, max(8, int(round(n ** 0.45)))), 2, seed=42)  # (d = 2: only the graph is used)
    e, truth = np.ascontiguousarray(g["edges"]), g["comm"][:, 0]
    print(f"\n== n {n}, m {len(e)}, planted communities {g['C']} (generated in {time.time() - t0:.1f} s)", flush=True)
    ctx = api.Context(0)
    ctx.set_graph(e, np.ones(len(e)), n)
    lv = ctx.louvain_levels()
    ctx.set_option("ecg_group", 0)
    base = ctx.ecg(K, W_MIN, SEED)
    for name, (comm, nc) in (("level 1", lv[0][:2]), (f"last level ({len(lv)})", lv[-1][:2]), ("ECG", base[:2])):
        print(f"quality  {name:16s} ARI {ari(comm, truth):.4f}  communities {nc}", flush=True)
    print(f"ECG: modularity {base[2]:.6f} (reweighted graph {base[3]:.6f}), member rounds {ctx.get_stat('ecg_member_rounds')}, "
          f"peel rounds {ctx.get_stat('ecg_peel_rounds')}, levels {ctx.get_stat('ecg_levels')}, default groups {ctx.get_stat('ecg_groups')}",
          flush=True)
    order = [0] + [x for x in groups if x != 0]
    members = ctx.ecg_members_test(K, SEED)
    for grp in order:  # warm-up of every form.  The members (unit weights: exact sums) must be the same bits from each; the final
        # partition is on real weights (w_min = 0.05), where float atomics may break a tie another way from call to call
        ctx.set_option("ecg_group", grp)
        again = ctx.ecg_members_test(K, SEED)
        assert all(np.array_equal(x, y) for x, y in zip(members, again)), grp
        r = ctx.ecg(K, W_MIN, SEED)
        print(f"ecg_group {grp:2d}: groups {ctx.get_stat('ecg_groups')}, communities {r[1]}, ARI {ari(r[0], truth):.4f}, modularity {r[2]:.6f}", flush=True)
    wall = {grp: [] for grp in order}
    for _ in range(reps):
        for grp in order:
            ctx.set_option("ecg_group", grp)
            t0 = time.perf_counter()
            ctx.ecg(K, W_MIN, SEED)
            wall[grp].append((time.perf_counter() - t0) * 1e3)
    for grp in order:
        print(f"whole call, ecg_group {grp:2d} ({'default' if grp == 0 else 'one member at a time' if grp == 1 else 'groups of ' + str(grp)}): "
              f"{spread(wall[grp])}", flush=True)
    ctx.profile_enable(True)
    for grp in (0, 1):
        ctx.set_option("ecg_group", grp)
        ms = {s: [] for s in STAGES}
        for _ in range(reps):
            ctx.profile_reset()
            ctx.ecg(K, W_MIN, SEED)
            prof = ctx.profile()
            for s in STAGES:
                ms[s].append(prof.get(s, {}).get("total_ms", float("nan")))
        print(f"stages, ecg_group {grp} (median of {reps}): " + " | ".join(f"{s[4:]} {np.median(ms[s]):.2f}" for s in STAGES) + " ms", flush=True)
    ctx.profile_enable(False)
    ctx.set_option("ecg_group", 0)
    ctx.close()
    return e


def guard(e, parent_lib, reps=10):
    out_dir = tempfile.mkdtemp()
    graph_file = os.path.join(out_dir, "ecg_guard_graph.npy")
    np.save(graph_file, e)
    script = os.path.join(ROOT, "profiles", "louvain_levels.py")
    sides = {}
    try:
        for side, lib in (("parent", parent_lib), ("this", "-")):
            p = subprocess.Popen([sys.executable, script, "--worker", lib, graph_file], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            assert p.stdout.readline().strip() == "ready", side
            sides[side] = (p, [])
        for _ in range(reps):
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
    t = {side: [float(r[0]) for r in rs] for side, (_, rs) in sides.items()}
    print("\n== guard: cge_louvain, whole call, one call a side in turn")
    for side in ("parent", "this"):
        print(f"{side:6s} build: {spread(t[side])}")
    bound = max(t["parent"]) + (max(t["parent"]) - min(t["parent"]))
    print(f"rule: this build's median {np.median(t['this']):.2f} ms against the parent's slowest + spread {bound:.2f} ms: "
          f"{'within' if np.median(t['this']) <= bound else 'OVER'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="1,2,4,8,16")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    from cge.jl_amd import api, synth

    e = None
    for n in [int(x) for x in a.sizes.split(",")]:
        e = one_size(api, synth, n, a.reps, [int(x) for x in a.groups.split(",")])
    if a.parent_lib:
        guard(e, a.parent_lib)


if __name__ == "__main__":
    main()
