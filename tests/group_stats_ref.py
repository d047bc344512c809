"""Long-double references, a-priori error bounds and seeded inputs for the statistics stage of a landmark split (weighted mean,
weight sum, covariance, projection, side sums), as the hook cge_group_stats_test returns them (tests/test_gpu_group_stats.py;
tests/test_group_stats_ref.py checks this module itself on the CPU).

Bounds, with u = 2^-53, k = rows of the group, y_j = (x_j - mean_dev) sqrt(w_j) -- valid for any summation order, no measured
constant enters:
    sw       |err| <= (k - 1) u sum w
    mean_c   |err| <= (k + 4) u sum_j w_j |x_jc| / sum w
    cov_ab   |err| <= (k + 8) u sum_j |y_ja| |y_jb|        (and cov is bitwise symmetric: the eigen-solver reads one triangle)
    z_j      |err| <= (d + 6) u sum_c |y_jc| |v_c|
    side sums: each of sum w x^2, sum w x, sum w within (k + 2) u times the sum of the absolute terms
Where a bound is 0 the value must be exact.  The covariance and the projection are centred on the mean the code under test
RETURNED, and the projection uses its vector, so every stage is judged on its own error.  Every element of every output is
compared.  A group whose weights are all zero has no mean (0 / 0 in the reference too) and is never generated."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
N_ROWS = 6000
LENS = (1, 2, 3, 15, 16, 17, 1, 33, 1023, 1024, 1025, 2049)  # several tasks in one 16-row wave, a chunk of 1024 rows +- 1, three chunks
CLASSES = ("integer", "offset", "wide_weights", "zero_columns", "identical_rows", "outlier")


def group_lengths(d):
    """The batch's groups in task order; beyond d = 129 the long groups stop at 300 rows (the long-double reference stays quick)."""
    return [min(k, 300) if d > 129 else k for k in LENS]


def make_problem(cls, d, seed=0):
    """(X (N_ROWS, d), w (N_ROWS,), ids (R,) int32 in random order, off (T + 1,) int32) of data class `cls` at width d"""
    rng = np.random.default_rng([seed, d, CLASSES.index(cls)])
    lens = group_lengths(d)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.permutation(N_ROWS)[: off[-1]].astype(np.int32)
    w = rng.integers(1, 41, N_ROWS).astype(np.float64)
    X = rng.standard_normal((N_ROWS, d)) * rng.uniform(0.2, 3.0, d) + 2.0 * rng.standard_normal((8, d))[rng.integers(0, 8, N_ROWS)]
    if cls == "offset":
        X = 1e3 + 1e-3 * rng.standard_normal((N_ROWS, d))
    elif cls == "wide_weights":
        w = np.exp(rng.uniform(-12.0, 12.0, N_ROWS))
        w[rng.random(N_ROWS) < 0.1] = 0.0
        w[ids[off[:-1]]] = np.exp(rng.uniform(-12.0, 12.0, len(lens)))  # no group of zero weights only
    elif cls == "zero_columns":
        X[:, rng.permutation(d)[: (d + 1) // 2]] = 0.0
    elif cls == "identical_rows":
        for t in range(len(lens)):
            X[ids[off[t]:off[t + 1]]] = X[ids[off[t]]]
    elif cls == "outlier":
        for t in range(len(lens)):
            X[ids[off[t] + lens[t] // 2]] *= 1e6
    return np.ascontiguousarray(X), w, ids, off


def make_sides(d, off, seed=0):
    """Random sides 0 / 1 / 2 per row; task 0 (one row) is in neither, task 3 has side 2 empty, task 4 side 1"""
    rng = np.random.default_rng([seed, d, 77])
    side = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=int(off[-1]), p=[0.2, 0.4, 0.4])
    side[off[0]:off[1]] = 0
    side[off[3]:off[4]] = 1
    side[off[4]:off[5]] = 2
    return side


def _gram(y):
    """y'y in long double, by column blocks on and above the diagonal (numpy has no BLAS for it), mirrored"""
    d = y.shape[1]
    out = np.empty((d, d), dtype=LD)
    for a in range(0, d, 64):
        out[a:a + 64, a:] = np.einsum("ja,jb->ab", y[:, a:a + 64], y[:, a:])
        out[a:, a:a + 64] = out[a:a + 64, a:].T
    return out


def ref_mean(X, w, ids, off):
    """(mean (T, d), sw (T,)) in long double, rounded to fp64 by the caller where it needs `mean_in`"""
    T = len(off) - 1
    mean, sw = np.empty((T, X.shape[1]), dtype=LD), np.empty(T, dtype=LD)
    for t in range(T):
        r = ids[off[t]:off[t + 1]]
        wl = w[r].astype(LD)
        sw[t] = wl.sum()
        mean[t] = (X[r].astype(LD) * wl[:, None]).sum(0) / sw[t]
    return mean, sw


def _ratio(err, bound):
    """max over the elements of |err| / bound; an error where the bound is 0 counts as infinite"""
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    bad = (bound == 0) & (err != 0)
    if bad.any() or not np.all(np.isfinite(err)):
        return float("inf")
    return float((err / np.where(bound == 0, 1, bound)).max())


def worst_ratios(X, w, ids, off, out, side=None, mean_given=False):
    """The worst error / bound of every statistic over all groups and elements: a dict sw, mean, cov, z (, ss, s, ws with
    `side`).  `out` is what the code under test returned (the keys of api.group_stats_test).  mean_given: the means were an
    input (sw is not produced and the mean itself is not judged here)."""
    T, d = len(off) - 1, X.shape[1]
    worst = {"cov": 0.0, "z": 0.0}
    if not mean_given:
        worst.update(sw=0.0, mean=0.0)
    if side is not None:
        worst.update(ss=0.0, s=0.0, ws=0.0)

    def note(key, err, bound):
        worst[key] = max(worst[key], _ratio(err, bound))

    for t in range(T):
        r = ids[off[t]:off[t + 1]]
        k = len(r)
        xl, wl = X[r].astype(LD), w[r].astype(LD)
        if not mean_given:
            sw = wl.sum()
            note("sw", out["sw"][t] - sw, (k - 1) * U * sw)
            wx = xl * wl[:, None]
            note("mean", out["mean"][t] - wx.sum(0) / sw, (k + 4) * U * np.abs(wx).sum(0) / sw)
        y = (xl - out["mean"][t].astype(LD)) * np.sqrt(wl)[:, None]
        ya = np.abs(y)
        note("cov", out["cov"][t] - _gram(y), (k + 8) * U * _gram(ya))
        v = out["vec"][t].astype(LD)
        note("z", out["z"][off[t]:off[t + 1]] - y @ v, (d + 6) * U * (ya @ np.abs(v)))
        if side is not None:
            sd = side[off[t]:off[t + 1]]
            for q in (1, 2):
                m = sd == q
                got = out["sums"][t, q - 1]
                t2, t1, t0 = wl[m, None] * xl[m] * xl[m], wl[m, None] * xl[m], wl[m]
                note("ss", got[:d] - t2.sum(0), (k + 2) * U * np.abs(t2).sum(0))
                note("s", got[d:2 * d] - t1.sum(0), (k + 2) * U * np.abs(t1).sum(0))
                note("ws", got[2 * d] - t0.sum(), (k + 2) * U * t0.sum())
    return worst


def numpy_stats(X, w, ids, off, side=None, mean_in=None):
    """The same statistics by plain fp64 numpy, in the layout of api.group_stats_test"""
    T, d = len(off) - 1, X.shape[1]
    out = {"mean": np.empty((T, d)), "sw": np.full(T, np.nan), "cov": np.empty((T, d, d)), "vec": np.empty((T, d)),
           "z": np.empty(int(off[-1])), "sums": None if side is None else np.zeros((T, 2, 2 * d + 1))}
    for t in range(T):
        r = ids[off[t]:off[t + 1]]
        x, wt = X[r], w[r]
        if mean_in is None:
            out["sw"][t] = wt.sum()
            out["mean"][t] = (x * wt[:, None]).sum(0) / out["sw"][t]
        else:
            out["mean"][t] = mean_in[t]
        y = (x - out["mean"][t]) * np.sqrt(wt)[:, None]
        c = y.T @ y
        out["cov"][t] = np.triu(c) + np.triu(c, 1).T
        out["vec"][t] = np.linalg.eigh(out["cov"][t])[1][:, -1]
        out["z"][off[t]:off[t + 1]] = y @ out["vec"][t]
        if side is not None:
            for q in (1, 2):
                m = side[off[t]:off[t + 1]] == q
                out["sums"][t, q - 1, :d] = (wt[m, None] * (x[m] * x[m])).sum(0)
                out["sums"][t, q - 1, d:2 * d] = (wt[m, None] * x[m]).sum(0)
                out["sums"][t, q - 1, 2 * d] = wt[m].sum()
    return out


def is_symmetric(cov):
    return np.array_equal(cov, np.swapaxes(cov, -1, -2))
