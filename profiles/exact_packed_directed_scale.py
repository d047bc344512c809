"""The packed form of a DIRECTED exact sweep (option "exact_packed_directed") at scale, and the guard of the paths it
must leave alone.  Stand-alone; reads nothing outside the tree.

    python3 profiles/exact_packed_directed_scale.py run <library of the parent commit> [--out FILE] [--only NAME,NAME..]
        the driver: every step below in a fresh child process under a time limit of its own, in order; it stops at the first
        step that fails, faults or runs out of time and writes what it has (default FILE:
        profiles/exact_packed_directed_scale.txt).  The driver itself never opens the device.
    python3 profiles/exact_packed_directed_scale.py step <n> <resident|packed|undirected_packed> [library file]
        one exact-mode score of synth.abcd_like(n, 10 n, 80, 16, seed=7, directed=..), seed 3, 10 000 samples: the sweep's
        time, the Chung-Lu iterations, "exact_matrix_bytes", the event timers of the power / fit / vect_B kernels and the fit's
        time per iteration; the last line is JSON.
    python3 profiles/exact_packed_directed_scale.py bench [library file]
        bench.py --gpus 1 --steps 10 --warmup 3 on that library; the last line is bench.py's JSON.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ME = os.path.abspath(__file__)
OWN = os.path.join("cge.jl_amd", "csrc", "build", "libcge_hip.so")


def step(n, mode, lib):
    import ctypes

    import numpy as np

    from cge.jl_amd import api, synth

    if lib:
        api._LIB_PATH = os.path.abspath(lib)
    directed = mode != "undirected_packed"
    out = {"n": n, "mode": mode, "library": os.path.relpath(api._LIB_PATH, ROOT)}
    g = synth.abcd_like(n, 10 * n, 80, 16, seed=7, directed=directed)
    ctx = api.Context(0)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    try:
        if mode == "packed":
            ctx.set_option("exact_packed_directed", 2)
        if mode == "undirected_packed":
            ctx.set_option("exact_packed", 1)
    except api.CGEError as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return

    def free_bytes():
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        rc = ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(f), ctypes.byref(t))
        return (int(f.value), int(t.value)) if rc == 0 else (None, None)

    def stat(key):
        try:
            return ctx.get_stat(key)
        except api.CGEError:
            return None

    out["free_bytes_before"], out["total_bytes"] = free_bytes()
    ctx.profile_select(("packed_gd", "packed_extrema", "pow_matrix", "pow_log2", "dist_matrix", "fit_symv", "fit_persistent", "bvec",
                        "auc_tally"))
    try:
        runs = 1 if n > 100000 else 2  # (the first run allocates; the large one is run once, with the timers)
        for r in range(runs):
            timed = r == runs - 1
            ctx.profile_enable(timed)
            ctx.profile_reset()
            t0 = time.perf_counter()
            res = ctx.score([], -1, directed=directed, seed=3, auc_samples=10000)
            out["wall_s"] = time.perf_counter() - t0
            out["sweep_ms"] = ctx.phase_ms().get("sweep")
    except api.CGEError as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return
    tr = ctx.last_trace
    out["kernels_ms"] = {k: round(v["total_ms"], 2) for k, v in ctx.profile().items() if v["launches"]}
    out.update(result=[float(x) for x in res], iters=[int(x) for x in tr["iters"]], fit_iterations=stat("fit_iterations"),
               exact_packed=stat("exact_packed"), exact_matrix_bytes=stat("exact_matrix_bytes"),
               fit_persistent_alphas=stat("fit_persistent_alphas"))
    if out["fit_iterations"] and "fit_symv" in out["kernels_ms"]:
        out["fit_ms_per_iteration"] = round(out["kernels_ms"]["fit_symv"] / out["fit_iterations"], 4)
    best = int(np.nanargmin(tr["div"]))
    out["invariants"] = bool(len(res) == 7 and np.all(np.isfinite(res)) and res[1] == tr["div"][best] and res[0] == 0.25 * (best + 1)
                             and abs(res[6] - 1.96 * np.sqrt(res[5] * (1.0 - res[5]) / 10000)) <= 1e-12 * res[6])
    out["free_bytes_after"] = free_bytes()[0]  # (the sweep's buffers are still held)
    ctx.close()
    print(json.dumps(out))


def bench(lib):
    import runpy

    from cge.jl_amd import api

    if lib:
        api._LIB_PATH = os.path.abspath(lib)
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"]
    os.chdir(ROOT)
    runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")


def run(parent, out_path, only):
    steps = [  # (name, arguments, time limit in seconds)
        ("directed 60000 resident, parent commit's build", ["step", "60000", "resident", parent], 420),
        ("directed 60000 resident, this build", ["step", "60000", "resident"], 420),
        ("directed 60000 packed, this build", ["step", "60000", "packed"], 420),
        ("directed 150000 default options, parent commit's build", ["step", "150000", "resident", parent], 300),
        ("directed 150000 packed, this build", ["step", "150000", "packed"], 1100),
    ]
    for r in range(2):  # the guard: each side in alternation
        steps += [(f"undirected 60000 packed, parent commit's build, round {r}", ["step", "60000", "undirected_packed", parent], 240),
                  (f"undirected 60000 packed, this build, round {r}", ["step", "60000", "undirected_packed"], 240),
                  (f"bench headline, parent commit's build, round {r}", ["bench", parent], 300),
                  (f"bench headline, this build, round {r}", ["bench"], 300)]
    if only:
        steps = [s for s in steps if any(o in s[0] for o in only)]
    lines = []
    ok = True
    for name, args, limit in steps:
        t0 = time.perf_counter()
        p = subprocess.Popen([sys.executable, ME] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        while True:  # (a line a minute while a long step runs)
            try:
                so, se = p.communicate(timeout=60)
                rc, last, err = p.returncode, ([ln for ln in so.splitlines() if ln.startswith("{")] or [""])[-1], se[-2000:]
                break
            except subprocess.TimeoutExpired:
                if time.perf_counter() - t0 > limit:
                    p.kill()
                    p.communicate()
                    rc, last, err = 124, "", "time limit"
                    break
                print(f"   ... {name}: {time.perf_counter() - t0:.0f} s", flush=True)
        lines += [f"## {name} (limit {limit} s, took {time.perf_counter() - t0:.0f} s, exit {rc})", last, ""]
        print(lines[-3], flush=True)
        print(last[:600], flush=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines))
        if rc != 0:  # nothing more is started on the device after a failure
            print(err, flush=True)
            ok = False
            break
    return 0 if ok else 1


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "step":
        step(int(a[1]), a[2], a[3] if len(a) > 3 else None)
    elif a and a[0] == "bench":
        bench(a[1] if len(a) > 1 else None)
    elif a and a[0] == "run":
        out_path = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "exact_packed_directed_scale.txt")
        only = a[a.index("--only") + 1].split(",") if "--only" in a else None
        sys.exit(run(a[1], out_path, only))
    else:
        print(__doc__)
        sys.exit(2)
