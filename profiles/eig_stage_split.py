"""eig_stage_timing.py for several batch sizes and repetitions in one process (CGE_EIG_DIAG is read once per process):
argv: <library file under csrc/build> <d> <T> [<T> ...].  Run once per stage: CGE_EIG_DIAG=1 (stop after the tridiagonalisation),
2 (+ multisection), 3 (+ inverse iteration), 0 / unset (everything).  Optional CGE_EIG_SPLIT_ROLES=v sets the testing knob
test_eig_roles (0 by placement, 1 identity, 2 reversed, 3 rotated) where the library has it.  Per T: REPS repetitions of 10
launches, the HIP-event time per launch of each."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cge.jl_amd import api  # noqa: E402

api._LIB_PATH = os.path.join(os.path.dirname(api._LIB_PATH), sys.argv[1])
d, Ts, REPS = int(sys.argv[2]), [int(t) for t in sys.argv[3:]], 5
ctx = api.Context()
roles = os.environ.get("CGE_EIG_SPLIT_ROLES")
if roles is not None:
    ctx.set_option("test_eig_roles", int(roles))
ctx.profile_enable(True)
for T in Ts:
    rng = np.random.default_rng(0)
    A = np.empty((T, d, d))
    for t in range(T):
        Y = rng.normal(size=(2 * d, d)) * rng.uniform(0.5, 2.0, size=d)
        A[t] = Y.T @ Y
    ctx.group_eig(A)
    ms = []
    for _ in range(REPS):
        ctx.profile_reset()
        for _ in range(10):
            ctx.group_eig(A)
        pr = ctx.profile()["group_eig"]
        ms.append(pr["total_ms"] / pr["launches"])
    print(f"{sys.argv[1]} roles={roles} CGE_EIG_DIAG={os.environ.get('CGE_EIG_DIAG', '0')} T={T} d={d}: ms per launch "
          + " ".join(f"{m:.4f}" for m in ms) + f"  min {min(ms):.4f} max {max(ms):.4f}", flush=True)
