"""A plain reference of cge_link_auc (include/cge_hip.h) for tests/test_gpu_link_auc.py, on top of tests/link_ref.py: numpy and
long double, nothing of the kernels.

Positives: the m rows of the edge list, in the list's order, p_e = p(src, dst) as listed (repeated rows repeat, a self loop is
p(i, i)).  Negatives NE: undirected, the pairs i < j that no row joins in either orientation; directed, the ordered pairs i != j
with no row i -> j.  less[e] = #{NE : p < p_e}, ties[e] = #{NE : p == p_e}; summary {W, L, Tq} in edge-list order in long double.

  table           p(a, b) for every ordered pair: link_ref.prob's long-double value rounded to fp64 -- the value cge_link_prob is
                  specified to give (within link_ref.BOUND of it; the CPU tests compare the two countings on ONE table, the GPU test
                  takes the table from the device's own cge_link_prob, so no bound enters either);
  counts          brute force on a table: the negatives' values sorted, two searches per positive;
  scheme          the device's bookkeeping restated: the thresholds sorted ascending with the permutation kept; every pair of the
                  walked tiles that is a pair of the model: below t_min -> one counter, above t_max -> nothing; otherwise lb / ub by
                  binary search, a pair level with a run of thresholds is dropped when it is a resident edge (an edge's own value
                  is always one of the thresholds: only there are the keys asked) and else counted in E at the run's start, and G
                  at ub; less = the inclusive prefix sum of G plus the counter, ties = E of the slot's run, both written back
                  through the permutation.  `part` of `nparts` takes the positions part, part + nparts, ... of the tile walk.
"""
import numpy as np

import link_ref as lr

LD = np.longdouble
TILE, SB = 128, 32  # the pair tiles and the super-blocks of their walk (mfma_tile.hpp)


def table(c):
    """(n, n) fp64: p(a, b) of every ordered pair of the case (the diagonal: dist = 0)."""
    n = len(c["X"])
    a, b = np.divmod(np.arange(n * n), n)
    return np.asarray(lr.prob(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], a, b), np.float64).reshape(n, n)


def negatives_mask(n, edges, directed):
    """(n, n) bool: the pairs of NE (undirected: in the upper triangle)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    joined = np.zeros((n, n), bool)
    joined[e[:, 0], e[:, 1]] = True
    if not directed:
        joined |= joined.T
        return np.triu(~joined, 1)
    return ~joined & ~np.eye(n, dtype=bool)


def n_neg_from_keys(n, edges, directed):
    """|NE| the way the device takes it: all pairs minus the distinct non-loop keys of the edge list."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    a, b = e[:, 0], e[:, 1]
    if not directed:
        a, b = np.minimum(a, b), np.maximum(a, b)
    keys = np.unique((a << 32) | b)
    distinct = int(((keys >> 32) != (keys & 0xffffffff)).sum())
    return (n * (n - 1) if directed else n * (n - 1) // 2) - distinct


def summary(less, ties, w=None):
    """{W, L, Tq} accumulated in the list's order in long double, rounded once each."""
    W, L, Tq = LD(0), LD(0), LD(0)
    ww = np.ones(len(less)) if w is None else np.asarray(w, np.float64)
    for we, a, b in zip(ww.astype(LD), np.asarray(less).astype(LD), np.asarray(ties).astype(LD)):
        W += we
        L += we * a
        Tq += we * b
    return float(W), float(L), float(Tq)


def counts(P, edges, directed):
    """Brute force on the table P: (less, ties, p_e, n_neg)."""
    n = len(P)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    neg = np.sort(P[negatives_mask(n, e, directed)])
    pe = P[e[:, 0], e[:, 1]]
    lo = np.searchsorted(neg, pe, side="left")
    hi = np.searchsorted(neg, pe, side="right")
    return lo.astype(np.int64), (hi - lo).astype(np.int64), pe, len(neg)


def tile_positions(n, directed):
    """{(I, J): position in the walk} of the 128 x 128 tiles that hold pairs: super-blocks of 32 x 32 tiles row-major (undirected:
    the upper ones), tiles row-major inside; the padding of a super-block has positions too."""
    nT = (n + TILE - 1) // TILE
    nS = (nT + SB - 1) // SB
    out = {}
    for I in range(nT):
        for J in (range(nT) if directed else range(I, nT)):
            SI, SJ = I // SB, J // SB
            sb = SI * nS + SJ if directed else SI * nS - SI * (SI - 1) // 2 + (SJ - SI)
            out[(I, J)] = sb * SB * SB + (I % SB) * SB + (J % SB)
    return out


def scheme(P, edges, directed, part=0, nparts=1):
    """The device's bookkeeping on the table P for one part: (less, ties, tiles walked)."""
    n = len(P)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    m = len(e)
    pe = P[e[:, 0], e[:, 1]]
    perm = np.argsort(pe, kind="stable")
    t = pe[perm]
    a, b = (e[:, 0], e[:, 1]) if directed else (np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1]))
    keys = set(((a << 32) | b).tolist())
    G, E = np.zeros(m, np.int64), np.zeros(m, np.int64)
    below = tiles = 0
    for (I, J), pos in tile_positions(n, directed).items():
        if pos % nparts != part:
            continue
        tiles += 1
        ii, jj = np.meshgrid(np.arange(I * TILE, min(n, (I + 1) * TILE)), np.arange(J * TILE, min(n, (J + 1) * TILE)), indexing="ij")
        ok = (ii != jj) if directed else (ii < jj)
        ii, jj = ii[ok], jj[ok]
        v = P[ii, jj]
        below += int((v < t[0]).sum())
        mid = (v >= t[0]) & (v <= t[-1])
        ii, jj, v = ii[mid], jj[mid], v[mid]
        lb = np.searchsorted(t, v, side="left")
        ub = np.searchsorted(t, v, side="right")
        level = lb < ub
        is_edge = np.array([lv and ((int(x) << 32) | int(y)) in keys for lv, x, y in zip(level, ii, jj)], bool)
        keep = ~is_edge
        np.add.at(E, lb[keep & level], 1)
        np.add.at(G, ub[keep & (ub < m)], 1)
    pref = np.cumsum(G) + below
    less, ties = np.zeros(m, np.int64), np.zeros(m, np.int64)
    run0 = np.searchsorted(t, t, side="left")
    less[perm] = pref
    ties[perm] = E[run0]
    return less, ties, tiles


# ---- the inputs the CPU and the GPU tests share --------------------------------------------------------------------------------------
def likely_edges(X, hi, alpha, fo, fi, m, seed, directed, repeats=True):
    """m rows (0-based) drawn among the pairs the model finds likely -- the upper half of an fp64 estimate of p, the top tenth
    left out -- so that non-edges exist on both sides of every positive: far pairs of small factors below the smallest, near
    pairs of large factors above the largest.  With `repeats`: a repeated row, its other orientation and a self loop."""
    n = len(X)
    rng = np.random.default_rng(seed)
    D = np.sqrt(np.maximum(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2), 0.0)) if n <= 300 else None
    if D is None:  # (n = 1000: the Gram form is enough for a choice of edges)
        sq = (X * X).sum(axis=1)
        D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))
    Pa = np.outer(fo, fo if fi is None else fi) * np.maximum(1.0 - D / hi, 0.0) ** alpha
    ok = ~np.eye(n, dtype=bool) if directed else np.triu(np.ones((n, n), bool), 1)
    ii, jj = np.nonzero(ok)
    v = Pa[ii, jj]
    lo, up = np.quantile(v, [0.5, 0.9]) if len(v) > 4 else (-np.inf, np.inf)
    pool = np.flatnonzero((v >= lo) & (v <= up))
    pick = rng.choice(pool, m, replace=len(pool) < m)
    e = np.stack([ii[pick], jj[pick]], axis=1)
    flip = rng.random(m) < 0.5
    if not directed:
        e[flip] = e[flip][:, ::-1]
    if repeats and m >= 8:
        e[1] = e[0]
        e[2] = e[0][::-1]
        e[3] = (e[3][0], e[3][0])
    return e.astype(np.int64)


# (n, d, m, directed, seed): every n and d of the issue, m from n - 1 to about 8 n, both orientations
AUC_SHAPES = [
    (2, 1, 1, False, 1),
    (2, 5, 1, True, 2),
    (129, 32, 128, False, 3),
    (129, 130, 1032, True, 4),
    (300, 5, 299, True, 5),
    (300, 130, 2400, False, 6),
    (300, 1, 1200, False, 7),
    (1000, 32, 8000, False, 8),
    (1000, 5, 999, True, 9),
]


def shape_case(n, d, m, directed, seed, alpha=2.25):
    """Points, factors spanning three decades (10^U(-1.5, 1.5)), hi = the diameter (n = 1000: twice the largest distance from the
    mean, at least the diameter), likely edges."""
    rng = np.random.default_rng(3000 + seed)
    X = lr.points(n, d, 100 + seed)
    hi = max(lr.diameter(X)[0], 1.0) if n <= 300 else 2.0 * float(np.sqrt(((X - X.mean(axis=0)) ** 2).sum(axis=1)).max())
    fo = 10.0 ** rng.uniform(-1.5, 1.5, n)
    fi = 10.0 ** rng.uniform(-1.5, 1.5, n) if directed else None
    edges = likely_edges(X, hi, alpha, fo, fi, m, seed, directed) if n > 2 else np.array([[1, 0]] * m, np.int64)
    return dict(X=X, hi=float(hi), alpha=float(alpha), fo=fo, fi=fi, edges=edges, directed=directed)


def stress_cases():
    c = {}
    rng = np.random.default_rng(79)
    # duplicated rows with equal factors: the positive (5, 7) and the negatives (105, 7), (5, 107), (105, 107) share a value to the
    # bit; so do many more
    X = lr.points(300, 8, 31)
    X[100:200] = X[0:100]
    fo = 10.0 ** rng.uniform(-1.0, 1.0, 300)
    fo[100:200] = fo[0:100]
    hi = lr.diameter(X)[0]
    e = likely_edges(X, hi, 2.25, fo, None, 600, 31, False)
    e = e[~((np.minimum(e[:, 0], e[:, 1]) % 100 == 5) & (np.maximum(e[:, 0], e[:, 1]) % 100 == 7))]
    e = np.r_[e, [[5, 7], [20, 120]]]  # (20, 120): a pair of duplicates, dist = 0
    c["ties_between_positives_and_negatives"] = dict(X=X, hi=hi, alpha=2.25, fo=fo, fi=None, edges=e, directed=False)
    X = lr.points(257, 17, 32)
    hi = lr.diameter(X)[0]
    one = np.ones(257)
    c["equal_factors"] = dict(X=X, hi=hi, alpha=3.0, fo=one, fi=None, edges=likely_edges(X, hi, 3.0, one, None, 700, 32, False), directed=False)
    # a zero factor: positives and negatives of p = 0 tie at 0, t_min = 0 (nothing is proven below)
    X = lr.points(200, 16, 33)
    hi = lr.diameter(X)[0]
    fo = 10.0 ** rng.uniform(-1.0, 1.0, 200)
    e = likely_edges(X, hi, 2.0, fo, None, 500, 33, False)
    fo[[3, 50, 130]] = 0.0
    e = np.r_[e, [[3, 9], [50, 130], [77, 3]]]
    c["zero_factor"] = dict(X=X, hi=hi, alpha=2.0, fo=fo, fi=None, edges=e, directed=False)
    # hi supplied below the diameter: clamped bases, many values 0
    for directed in (False, True):
        k = shape_case(300, 5, 900, directed, 34 + directed)
        k["hi"] = 0.5 * lr.diameter(k["X"])[0]
        k["edges"] = np.r_[likely_edges(k["X"], k["hi"], k["alpha"], k["fo"], k["fi"], 900, 34, directed), lr.random_edges(300, 40, 34, directed)]
        c[f"small_hi_dir{int(directed)}"] = k
    # complete graphs: no negatives at all
    X = lr.points(40, 5, 36)
    ii, jj = np.triu_indices(40, 1)
    c["complete"] = dict(X=X, hi=lr.diameter(X)[0], alpha=2.0, fo=10.0 ** rng.uniform(-1, 1, 40), fi=None, edges=np.stack([jj, ii], axis=1),
                         directed=False)
    ii, jj = np.nonzero(~np.eye(40, dtype=bool))
    c["complete_directed"] = dict(X=X, hi=lr.diameter(X)[0], alpha=2.0, fo=10.0 ** rng.uniform(-1, 1, 40), fi=10.0 ** rng.uniform(-1, 1, 40),
                                  edges=np.stack([ii, jj], axis=1), directed=True)
    # a star: every positive shares the hub
    X = lr.points(300, 32, 37)
    leaves = np.delete(np.arange(300), 17)
    c["star"] = dict(X=X, hi=lr.diameter(X)[0], alpha=2.25, fo=10.0 ** rng.uniform(-1.5, 1.5, 300), fi=None,
                     edges=np.stack([np.full(299, 17), leaves], axis=1), directed=False)
    for alpha in (0.25, 10.0):
        c[f"alpha_{alpha}"] = shape_case(300, 32, 1500, False, 38, alpha=alpha)
    return {k: dict(v, edges=np.asarray(v["edges"], np.int64).reshape(-1, 2)) for k, v in c.items()}


# ---- the fitted models of the statistical test -----------------------------------------------------------------------------------
# (fixture, land, seed of the score, auc_samples): element 6 of the vector is the mean of S Bernoulli(q) draws, q = local_exact
FITTED = [("test115", 20, 17, 2000), ("test115", -1, 23, 2000), ("abcd2000", 60, 17, 4000), ("abcd2000", -1, 29, 4000)]
SIGMAS = 5.0


def within_sigmas(estimate, q, S):
    """|estimate - q| <= 5 sqrt(q (1 - q) / S): the issue's condition."""
    return abs(estimate - q) <= SIGMAS * np.sqrt(q * (1.0 - q) / S)
