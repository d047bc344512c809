"""The packed form of an exact sweep (option "exact_packed") at scale: `python3 profiles/exact_packed_scale.py n packed|resident|auto
[library file]` scores synth.abcd_like(n, 10 n, 80, 16, seed=7) in exact mode (seed 3, 10 000 samples) and prints the sweep's
time, its iterations, the O(N^2) bytes it required and the power kernels' event timers; the last line is JSON.  `auto` leaves the
options at their defaults (and checks the invariants of test_exact_mode_sixty_thousand_vertices); an alternative library file
(another build, for the A/B) is loaded when given."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cge.jl_amd import api, synth  # noqa: E402

n, mode = int(sys.argv[1]), sys.argv[2]
if len(sys.argv) > 3:
    api._LIB_PATH = os.path.abspath(sys.argv[3])
out = {"n": n, "mode": mode, "library": os.path.relpath(api._LIB_PATH, ROOT)}
g = synth.abcd_like(n, 10 * n, 80, 16, seed=7)
ctx = api.Context(0)
ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
if mode == "packed":
    ctx.set_option("exact_packed", 1)


def free_bytes():
    """hipMemGetInfo of the context's device, asked of the runtime the library loaded."""
    import ctypes

    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    rc = ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(f), ctypes.byref(t))
    return (int(f.value), int(t.value)) if rc == 0 else (None, None)


out["free_bytes_before"], out["total_bytes"] = free_bytes()


def stat(key):
    try:
        return ctx.get_stat(key)
    except api.CGEError:
        return None  # a build without the stat


runs = 1 if mode == "auto" else 2
try:
    for r in range(runs):  # (the first run allocates)
        t0 = time.perf_counter()
        res = ctx.score([], -1, seed=3, auc_samples=10000)
        out["wall_s"] = time.perf_counter() - t0
        out["sweep_ms"] = ctx.phase_ms().get("sweep")
except api.CGEError as e:
    out["error"] = str(e)
    print(json.dumps(out))
    sys.exit(0)
tr = ctx.last_trace
out.update(result=[float(x) for x in res], iters=[int(x) for x in tr["iters"]], fit_iterations=stat("fit_iterations"),
           exact_packed=stat("exact_packed"), exact_matrix_bytes=stat("exact_matrix_bytes"),
           fit_persistent_alphas=stat("fit_persistent_alphas"))
best = int(np.nanargmin(tr["div"]))
out["invariants"] = bool(len(res) == 7 and np.all(np.isfinite(res)) and res[1] == tr["div"][best] and res[0] == 0.25 * (best + 1)
                         and abs(res[6] - 1.96 * np.sqrt(res[5] * (1.0 - res[5]) / 10000)) <= 1e-12 * res[6])
if mode != "auto":  # once more with the event timers of the power and the fit
    ctx.profile_select(("packed_gd", "packed_extrema", "pow_matrix", "pow_log2", "dist_matrix", "fit_symv", "bvec"))
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.score([], -1, seed=3, auc_samples=10000)
    out["timed_sweep_ms"] = ctx.phase_ms().get("sweep")
    out["kernels_ms"] = {k: round(v["total_ms"], 2) for k, v in ctx.profile().items() if v["launches"]}
out["free_bytes_after"] = free_bytes()[0]  # (the sweep's buffers are still held)
ctx.close()
print(json.dumps(out))
