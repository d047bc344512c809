"""The Chung-Lu fixed point of wGCL / wGCL_directed, written from the reference's loops (oracle/cge_oracle.c:848-865 undirected,
:1031-1055 directed; src/divergence.jl:150-168, :434-467), on a GIVEN power matrix GD and from a GIVEN start, with the whole
trajectory returned -- and the seeded problems tests/test_gpu_fit.py runs on the device.  No GPU is needed here.

  undirected  S_i = sum_j (T_i T_j) GD_ij;  T_i += eps T_i (w_i / S_i - 1);  f = max_i |w_i - S_i|;  while f > delta
  directed    Sin_i = sum_j (Tin_i Tout_j) GD_ij, Sout_i = sum_j (Tin_j Tout_i) GD_ij, the j == i term counted TWICE in both (the
              reference's inner loop runs j = i..N and adds tmp1 and tmp2 at j == i); rows with deg > 0 only are updated and
              enter f (the others keep their value bit for bit); `if f > diff: epsilon *= 0.99` AFTER the update, diff starts at 1.0

dtype np.longdouble: the reference proper (sums as matrix-vector products, 64-bit significand).  dtype np.float64: the same
iteration in plain fp64 IN THE ORACLE'S SUMMATION ORDER -- S_i is a left-to-right sum over j = 0..N-1 of (T_i T_j) GD_ij (its
i-major pair loop reaches S_i from the rows above first, then along row i), the directed diagonal term twice in a row.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53


def symmetric(GD_upper):
    """The full symmetric matrix of a matrix given for j >= i (anything, NaN included, below the diagonal)."""
    G = np.triu(np.asarray(GD_upper))
    return G + np.triu(G, 1).T


def _seq_rows(M):
    """Left-to-right sums of the rows of M (np.cumsum is strictly sequential)."""
    return np.cumsum(M, axis=1)[:, -1]


_ROWS = 128  # rows per block of the fp64 sums (the blocks stay in cache)


def sums_undirected(GD, T, dtype):
    if dtype is LD:
        return T * (GD @ T)
    S = np.empty(T.size)
    for a in range(0, T.size, _ROWS):
        b = min(T.size, a + _ROWS)
        S[a:b] = _seq_rows((T[a:b, None] * T[None, :]) * GD[a:b])
    return S


def sums_directed(GD, Tin, Tout, dtype):
    d = np.diagonal(GD)
    if dtype is LD:
        return Tin * (GD @ Tout + d * Tout), Tout * (GD @ Tin + d * Tin)
    N = Tin.size
    Sin, Sout = np.empty(N), np.empty(N)
    M2 = np.empty((_ROWS, N + 1))

    def twice(M, a):  # row i: columns 0..i, column i AGAIN, columns i+1..N-1
        m = M2[:M.shape[0]]
        m[:, -1] = 0.0
        m[:, :-1] = np.tril(M, a)
        m[:, 1:] += np.triu(M, a)  # (onto zeros: exact)
        return m

    for a in range(0, N, _ROWS):
        b = min(N, a + _ROWS)
        Sin[a:b] = _seq_rows(twice((Tin[a:b, None] * Tout[None, :]) * GD[a:b], a))
        Sout[a:b] = _seq_rows(twice((Tin[None, :] * Tout[a:b, None]) * GD[a:b], a))
    return Sin, Sout


def fit_undirected(GD, T0, w, eps, delta=None, steps=None, dtype=LD, max_iters=100000):
    """GD: full symmetric (N, N).  Exactly `steps` iterations, or `while f > delta`.  Returns a dict: T = [T_0 .. T_K],
    S = [S_0 .. S_{K-1}], f = [f_0 .. f_{K-1}], eps = [eps] * K, iters = K."""
    assert (delta is None) != (steps is None)
    GD, T, w, eps = np.asarray(GD, dtype=dtype), np.asarray(T0, dtype=dtype).copy(), np.asarray(w, dtype=dtype), dtype(eps)
    out = {"T": [T.copy()], "S": [], "f": [], "eps": []}
    diff = 1.0
    while (len(out["f"]) < steps) if steps is not None else (diff > delta):
        S = sums_undirected(GD, T, dtype)
        T = T + (eps * T) * (w / S - dtype(1))
        diff = np.max(np.abs(w - S))
        out["T"].append(T.copy()); out["S"].append(S); out["f"].append(diff); out["eps"].append(eps)
        assert len(out["f"]) <= max_iters, "no convergence"
    out["iters"] = len(out["f"])
    return out


def fit_directed(GD, Tin0, Tout0, deg_in, deg_out, eps, delta=None, steps=None, dtype=LD, max_iters=100000):
    """As fit_undirected; T = [(Tin_k, Tout_k)], S = [(Sin_k, Sout_k)], eps[k] = the epsilon iteration k moved with."""
    assert (delta is None) != (steps is None)
    GD = np.asarray(GD, dtype=dtype)
    Tin, Tout = np.asarray(Tin0, dtype=dtype).copy(), np.asarray(Tout0, dtype=dtype).copy()
    din, dout, eps = np.asarray(deg_in, dtype=dtype), np.asarray(deg_out, dtype=dtype), dtype(eps)
    mi, mo = din > 0, dout > 0
    out = {"T": [(Tin.copy(), Tout.copy())], "S": [], "f": [], "eps": []}
    diff = dtype(1.0)
    while (len(out["f"]) < steps) if steps is not None else (diff > delta):
        Sin, Sout = sums_directed(GD, Tin, Tout, dtype)
        Tin, Tout = Tin.copy(), Tout.copy()
        Tin[mi] = Tin[mi] + (eps * Tin[mi]) * (din[mi] / Sin[mi] - dtype(1))
        Tout[mo] = Tout[mo] + (eps * Tout[mo]) * (dout[mo] / Sout[mo] - dtype(1))
        f = max(np.max(np.abs(din[mi] - Sin[mi]), initial=dtype(0)), np.max(np.abs(dout[mo] - Sout[mo]), initial=dtype(0)))
        out["T"].append((Tin.copy(), Tout.copy())); out["S"].append((Sin, Sout)); out["f"].append(f); out["eps"].append(eps)
        if f > diff:
            eps = eps * dtype(0.99)
        diff = f
        assert len(out["f"]) <= max_iters, "no convergence"
    out["iters"] = len(out["f"])
    return out


def delta_for(f, K):
    """The threshold that ends a fit with the f trajectory `f` at exactly K iterations: the geometric mean of f_{K-1} and the
    smallest earlier f (K == 1: twice f_0).  Returns (delta, gap): gap = the factor between the two values that bracket it."""
    f = [float(x) for x in f]
    if K == 1:
        return 2.0 * f[0], 2.0
    lo, hi = f[K - 1], min(f[:K - 1])
    return float(np.sqrt(lo * hi)), hi / lo


def rel_dist(a, b):
    """The largest relative distance of a from b (elements where b is 0 must agree exactly)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    nz = b != 0
    assert np.array_equal(a[~nz], b[~nz])
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]), initial=0.0))


# ---- the problems ------------------------------------------------------------------------------------------------------

def distances(N, seed):
    """Pairwise Euclidean distances of N normal points in 4 dimensions over their maximum: symmetric, zero diagonal, one pair
    at exactly 1 (so GD holds an exact 0) from two vertices on."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, 4))
    D = np.sqrt(np.maximum(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1), 0.0)) if N <= 1024 else _big_dist(X)
    D = np.maximum(D, D.T)
    np.fill_diagonal(D, 0.0)
    m = D.max()
    return D / m if m > 0 else D


def _big_dist(X):
    g = (X * X).sum(1)
    return np.sqrt(np.maximum(g[:, None] + g[None, :] - 2.0 * (X @ X.T), 0.0))


def _zero_rows(rng, N, k):
    return rng.choice(N, size=k, replace=False) if N >= 8 else np.zeros(0, dtype=np.int64)


def random_undirected(N, alpha, seed):
    """D, alpha, w: the weights are the sums of a hidden iterate exp(normal) times 1 + 0.3 U(-1, 1); two rows (N >= 8) have
    weight 0."""
    D = distances(N, seed)
    rng = np.random.default_rng(seed + 1000003)
    GD = (1.0 - D) ** alpha
    Th = np.exp(rng.normal(size=N))
    w = Th * (GD @ Th) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=N))
    w[_zero_rows(rng, N, 2)] = 0.0
    return {"D": D, "alpha": float(alpha), "w": w, "T0": np.ones(N)}


def random_directed(N, alpha, seed):
    """D, alpha, deg_in (w), deg_out (w2) from hidden Tin, Tout; two rows (N >= 8) have deg_in 0 and two OTHERS deg_out 0.  The
    start is the sweep's: 1, and 0 where the degree is 0."""
    D = distances(N, seed)
    rng = np.random.default_rng(seed + 2000003)
    GD = (1.0 - D) ** alpha
    Ti, To = np.exp(rng.normal(size=N)), np.exp(rng.normal(size=N))
    d = np.diagonal(GD)
    din = Ti * (GD @ To + d * To) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=N))
    dout = To * (GD @ Ti + d * Ti) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=N))
    z = _zero_rows(rng, N, 4)
    din[z[:2]] = 0.0
    dout[z[2:]] = 0.0
    return {"D": D, "alpha": float(alpha), "w": din, "w2": dout, "T0": (din > 0).astype(np.float64),
            "T0b": (dout > 0).astype(np.float64)}


def exact_problem(N, seed, directed):
    """Inputs on which every product and every sum of one iteration is exact in fp64 in any order: D in {0, 1/4, 1/2, 3/4, 1}
    (zero diagonal) at alpha = 1, the start in {0.5, 1, 1.5, 2}, and weights w_i = S_i r_i with r_i in {1/2, 1, 3/2, 2}, so that
    w / S, the move (eps a power of two) and T_1 are exact too.  Directed: rows 1 and 3 (N >= 8) have deg_in 0, rows 2 and 5
    deg_out 0.  Returns (problem, T_1 or (Tin_1, Tout_1), f_0) with eps = 0.25 undirected, 0.5 directed."""
    rng = np.random.default_rng(seed)
    D = np.triu(rng.integers(0, 5, size=(N, N)).astype(np.float64) / 4.0, 1)
    D = D + D.T
    GD = 1.0 - D
    vals = np.array([0.5, 1.0, 1.5, 2.0])
    pr = {"D": D, "alpha": 1.0}
    if not directed:
        T0, r = vals[rng.integers(0, 4, N)], vals[rng.integers(0, 4, N)]
        S = T0 * (GD @ T0)
        _assert_exact(S, 16.0)
        w = S * r
        pr.update(w=w, T0=T0)
        return pr, T0 + (0.25 * T0) * (w / S - 1.0), float(np.max(np.abs(w - S)))
    Ti, To = vals[rng.integers(0, 4, N)], vals[rng.integers(0, 4, N)]
    ri, ro = vals[rng.integers(0, 4, N)], vals[rng.integers(0, 4, N)]
    d = np.diagonal(GD)
    Sin, Sout = Ti * (GD @ To + d * To), To * (GD @ Ti + d * Ti)
    _assert_exact(Sin, 16.0); _assert_exact(Sout, 16.0)
    din, dout = Sin * ri, Sout * ro
    if N >= 8:
        din[[1, 3]] = 0.0
        dout[[2, 5]] = 0.0
    mi, mo = din > 0, dout > 0
    Ti1, To1 = Ti.copy(), To.copy()
    Ti1[mi] = Ti[mi] + (0.5 * Ti[mi]) * (din[mi] / Sin[mi] - 1.0)
    To1[mo] = To[mo] + (0.5 * To[mo]) * (dout[mo] / Sout[mo] - 1.0)
    f0 = max(np.max(np.abs(din[mi] - Sin[mi]), initial=0.0), np.max(np.abs(dout[mo] - Sout[mo]), initial=0.0))
    pr.update(w=din, w2=dout, T0=Ti, T0b=To)
    return pr, (Ti1, To1), float(f0)


def _assert_exact(S, scale):
    """From the magnitudes: every term is a multiple of 1 / scale and the sums stay far below 2^53 / scale, so fp64 adds them
    exactly in any order."""
    assert np.all(S * scale == np.round(S * scale)) and np.max(S) * scale < 2.0 ** 50


def step_bound(eps, T_prev, w, S_prev, T_next, N):
    """A-priori bound on |T_dev - T_ld| after ONE device step from T_prev in fp64, any order of additions, any mix of FMAs
    (u = 2^-53).  All terms of S_i are non-negative and carry at most three roundings each, so S_dev = S (1 + t), |t| <= (N + 3) u;
    the quotient, the subtraction, eps T and the product add one rounding each: the move is off by at most
    eps T u ((N + 4) w/S + 3 |w/S - 1|), the final addition by u |T_next|.  Stated (and asserted) in the rounder form
        eps T (N + 8) u (w/S + |w/S - 1|) + 2 u |T_next|.
    Rows with w == 0 that the directed fit skips have T_next == T_prev and are compared for equality by the caller."""
    eps, T_prev, w, S_prev, T_next = (np.asarray(x, dtype=LD) for x in (eps, T_prev, w, S_prev, T_next))
    r = np.divide(w, S_prev, out=np.zeros_like(w), where=w > 0)  # (w == 0: the quotient is 0, or the row is skipped)
    return eps * np.abs(T_prev) * LD(N + 8) * U * (r + np.abs(r - 1)) + 2 * U * np.abs(T_next)


# ---- the K-step cases of tests/test_gpu_fit.py (V3): chains of fits, as a sweep runs them ------------------------------------
# A chain is one problem (N, seed) fitted at a list of (alpha, K, start): start "ones" = the sweep's start, "prev" = the iterate
# the previous case of the chain ended on (at the same alpha: the fit goes on; at another: what a sweep does).  K: an iteration
# count; "conv" = whatever delta = 1e-3 gives; ("rec", t) = the first running-minimum record of f at or after iteration t
# (pick_record: from a previous iterate at another alpha, and in the directed zig-zag, f is not monotone).
def _rec(t):
    return ("rec", t)


_BIG_U = [(1.0, 2, "ones"), (1.0, 3, "prev")]
_BIG_D = [(1.0, 3, "ones"), (1.0, 2, "prev")]
UNDIRECTED_CHAINS = {
    # every K from 1 to 13: each residue of the rings of length 2, 3, 4 (and of their common period 12) ends a fit
    65: (101, [(1.0, "conv", "ones"), (1.0, 1, "prev"), (1.25, _rec(2), "prev"), (1.5, _rec(13), "prev"), (4.0, 4, "ones"),
               (4.0, 3, "prev"), (4.0, 5, "prev"), (4.0, 6, "prev"), (4.0, 7, "prev"), (4.0, 8, "prev"), (4.0, 9, "prev"), (4.0, 10, "prev"), (4.0, 11, "prev"),
               (4.0, 12, "prev")]),
    130: (102, [(4.0, "conv", "ones"), (4.25, _rec(3), "prev"), (4.5, _rec(5), "prev"), (4.75, _rec(25), "prev"), (2.0, 2, "ones")]),
    700: (103, [(10.0, "conv", "ones"), (9.75, _rec(4), "prev"), (9.5, _rec(13), "prev"), (1.0, _rec(3), "ones"), (1.0, 25, "prev")]),
    1985: (104, _BIG_U), 2816: (105, [(1.0, 3, "ones"), (1.0, 2, "prev")]), 2817: (106, _BIG_U),
    4032: (107, [(1.0, 3, "ones"), (1.0, 2, "prev")]), 4097: (108, _BIG_U),
}
DIRECTED_CHAINS = {
    65: (201, [(4.0, _rec(6), "ones"), (4.25, _rec(2), "prev"), (4.5, _rec(2), "prev")]),
    130: (202, [(1.0, _rec(12), "ones"), (1.25, _rec(3), "prev"), (1.5, _rec(3), "prev")]),  # the first: the DESIGNATED case
    700: (203, [(4.0, _rec(8), "ones"), (4.25, _rec(2), "prev")]),
    1985: (204, _BIG_D), 2816: (205, _BIG_D), 2817: (206, _BIG_D), 4032: (207, _BIG_D), 4097: (208, _BIG_D),
}
DESIGNATED_DIRECTED = 130
# the sizes that tests/test_gpu_small_chip_fits.py adds for the geometries of chips with 2 .. 64 CUs (130 takes its chain above):
# long chains while a long-double step is cheap, two short ones (one from ones, one from the previous end) beyond
SMALL_CHIP_UNDIRECTED_CHAINS = {
    7: (111, [(1.0, "conv", "ones"), (1.25, _rec(2), "prev"), (4.0, 3, "ones")]),
    64: (112, [(4.0, "conv", "ones"), (4.25, _rec(3), "prev"), (2.0, 2, "ones")]),
    256: (113, [(4.0, "conv", "ones"), (4.25, _rec(3), "prev"), (4.5, _rec(13), "prev"), (2.0, 2, "ones")]),
    513: (114, [(10.0, "conv", "ones"), (9.75, _rec(4), "prev"), (1.0, _rec(3), "ones")]),
    960: (115, [(1.0, 3, "ones"), (1.0, _rec(4), "prev")]), 961: (116, [(1.0, 4, "ones"), (1.0, 3, "prev")]),
    1024: (117, [(1.0, 3, "ones"), (1.0, _rec(5), "prev")]), 1409: (118, _BIG_U),
}
SMALL_CHIP_DIRECTED_CHAINS = {
    7: (211, [(4.0, _rec(6), "ones"), (4.25, _rec(2), "prev")]),
    64: (212, [(1.0, _rec(12), "ones"), (1.25, _rec(3), "prev")]),
    256: (213, [(1.0, _rec(12), "ones"), (1.25, _rec(3), "prev")]),
    513: (214, [(4.0, _rec(8), "ones"), (4.25, _rec(2), "prev")]),
    960: (215, _BIG_D), 961: (216, _BIG_D), 1024: (217, _BIG_D), 1409: (218, _BIG_D),
}
GAP = 1.1       # the least factor between the two values of f that bracket a case's delta (asserted of every case)
PICK_GAP = 1.2  # ... and the factor a record is picked by, so that no pick sits on the edge of GAP


def pick_record(f, target):
    """The first K >= target at which f_{K-1} is a running-minimum record by the factor PICK_GAP (K == 1 always is)."""
    f = [float(x) for x in f]
    for K in range(max(1, target), len(f) + 1):
        if K == 1 or f[K - 1] * PICK_GAP <= min(f[:K - 1]):
            return K
    raise AssertionError("no record of the zig-zag at or after iteration %d" % target)


def chain_cases(N, directed, gd_of, tables=None):
    """The cases of the chain of N (of `tables` = (undirected, directed), else of the tables of test_gpu_fit.py) with their
    long-double references.  gd_of(problem, alpha) -> the full symmetric power matrix
    the references run on (the device's own on the GPU, numpy's on the CPU).  Yields dicts: problem (with alpha and the start),
    K, delta, gap, eps, ref (the long-double trajectory of exactly K steps), A (the amplification max(2, 2 E64(K) / E64(1)) of
    the one-step bound, E64(k) = the relative distance of the plain fp64 iteration from the long-double one after k steps),
    decays (directed: the iterations before K after which epsilon decayed)."""
    seed, chain = (tables or (UNDIRECTED_CHAINS, DIRECTED_CHAINS))[1 if directed else 0][N]
    base = (random_directed if directed else random_undirected)(N, chain[0][0], seed)  # (the hidden iterate: at the first alpha)
    eps = 0.9 if directed else 0.25
    prev = None
    out = []
    for alpha, K, start in chain:
        pr = dict(base, alpha=float(alpha))
        if start == "prev":
            if directed:
                pr["T0"], pr["T0b"] = (np.asarray(t, dtype=np.float64) for t in prev)
            else:
                pr["T0"] = np.asarray(prev, dtype=np.float64)
        GD = gd_of(pr, alpha)
        if directed:
            args = (GD, pr["T0"], pr["T0b"], pr["w"], pr["w2"], eps)
            fit = fit_directed
        else:
            args = (GD, pr["T0"], pr["w"], eps)
            fit = fit_undirected
        if K == "conv":
            K = fit(*args, delta=1e-3)["iters"]
        elif isinstance(K, tuple):
            K = pick_record(fit(*args, steps=K[1] + 12)["f"], K[1])
        ref = fit(*args, steps=K)
        delta, gap = delta_for(ref["f"], K)
        r64 = fit(*args, steps=K, dtype=np.float64)
        flat = (lambda t: np.concatenate(t)) if directed else (lambda t: t)
        e1, eK = rel_dist(flat(r64["T"][1]), flat(ref["T"][1])), rel_dist(flat(r64["T"][K]), flat(ref["T"][K]))
        decays = [k for k in range(K - 1) if ref["eps"][k + 1] < ref["eps"][k]] if directed else []
        out.append({"problem": pr, "K": K, "delta": delta, "gap": gap, "eps": eps, "ref": ref, "A": max(2.0, 2.0 * eK / e1),
                    "E64": (e1, eK), "decays": decays, "start": start})
        prev = ref["T"][K]
    return out


def numpy_gd(pr, alpha):
    return (1.0 - pr["D"]) ** alpha
