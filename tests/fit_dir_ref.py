"""A directed Chung-Lu problem that HAS a fixed point, for tests/test_gpu_fit_dir_tiles.py: fit_ref.random_directed perturbs the
two degree vectors independently (their totals differ, so its fits are stopped by a chosen delta, never by convergence); here the
degrees are the sums of a hidden (Tin, Tout) themselves, and the fit from the sweep's start converges to delta = 1e-3.  No GPU is
needed here."""
import numpy as np

import fit_ref as fr


def consistent_directed(N, alpha, seed):
    """fit_ref.random_directed's D at `alpha` with deg_in = Sin(Ti, To), deg_out = Sout(Ti, To) of a hidden iterate exp(N(0, 1/4));
    two rows have deg_in 0 and two others deg_out 0 (their hidden T is 0).  The start is the sweep's: 1, and 0 where the degree is 0."""
    pr = fr.random_directed(N, alpha, seed)
    rng = np.random.default_rng(seed + 7)
    GD = (1.0 - pr["D"]) ** alpha
    Ti, To = np.exp(0.5 * rng.normal(size=N)), np.exp(0.5 * rng.normal(size=N))
    z = rng.choice(N, 4, replace=False)
    Ti[z[:2]] = 0.0
    To[z[2:]] = 0.0
    Sin, Sout = fr.sums_directed(GD, Ti, To, fr.LD)
    pr["w"], pr["w2"] = np.asarray(Sin, np.float64), np.asarray(Sout, np.float64)
    pr["T0"], pr["T0b"] = (pr["w"] > 0).astype(np.float64), (pr["w2"] > 0).astype(np.float64)
    return pr
