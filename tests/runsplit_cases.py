"""Inputs for the tests of runsplit's host driver (tests/test_gpu_runsplit_driver.py; pinned on the CPU by
tests/test_runsplit_cases.py): seeded generators of small embeddings with clusters, at the shapes where the driver -- the
speculative expansion of advance_heaps, the replay, the held-back errors, the forced phase, the merge -- takes its branches.

Every case has integer coordinates and power-of-two weights.  The column sums sum w x^2, sum w x and sum w of any group are then
exact in any order of summation, a group's heap value -(sum_c ss - s^2 / ws) is the same expression of the same numbers on the
device and in the oracle, and two groups tie in value exactly when their values are equal numbers.

  tied      a 64-point pattern copied into 12 clusters; cluster q is the pattern translated by 64 q along the first axis.  The
            pattern's points are distinct integer points of [-8, 8]^3 that lie in the plane x0 = 0: a translation along an axis
            with spread would change s^2 / ws by an integer and the ROUNDING of the quotient with it, so the clusters' values
            would agree to some 1e-7 and not tie; along an axis without spread the column's term is exactly 0 before and after, and
            every cluster repeats the others' values bit for bit at every level of the tree.  The d = 1 variant (repeated
            coordinates: ties among the projections as well) has only that one axis, so there the 12 clusters are plain copies.
  blocks    150 distinct integer points of [-64, 64]^2, no two of them on a common diagonal, each repeated 1 to 4 times, shuffled,
            all weights 2.0, two clusters (the halves): blocks of equal rows are homogeneous groups of value 0, which `rss`
            refuses when (and only when) it pops them.  (A group {a, a, b} has the principal axis a - b exactly; on a common
            diagonal its two components have the same magnitude, and which of them the sign rule makes positive -- so which
            child is `low` -- hangs on the eigen-routine's last bits.  In [-16, 16]^2 at most 64 points avoid each other's
            diagonals, and without that no seed survives jittered eigenvectors: see blocks())
  distinct  150 such points, once each, in one cluster: nothing fails before a singleton is on top of the heap
  forced    clusters of 1, 2, 3, forced, forced + 1, 40 and 300 rows, neither the clusters nor their members in ascending order
"""
import numpy as np

RULES = ("rss", "rss2", "size", "diameter")
OK, E_ASSERT, E_HOMOGENEOUS, E_EMPTY = 0, -1, -2, -3
TIED_CLUSTERS, TIED_POINTS = 12, 64
TIED_FORCED = (1, 2, 4)
FORCED_VALUES = (1, 2, 3, 6)


class Case:
    """X (n, d) float64, w (n,), clusters (lists of 1-based ids, as runsplit takes them), forced, and the `land` values to run"""

    def __init__(self, name, X, w, clusters, forced, lands):
        self.name, self.X, self.w, self.clusters, self.forced, self.lands = name, X, w, clusters, forced, tuple(lands)
        self.n, self.d = X.shape
        self.edges = np.array([[1, 2]], dtype=np.int64)  # the landmark split never reads the graph
        self.comm = np.ones((self.n, 1), dtype=np.int64)

    def __repr__(self):
        return self.name


def _distinct_points(rng, count, lo, hi, d):
    side = hi - lo + 1
    flat = rng.choice(side ** d, size=count, replace=False)
    return np.stack([(flat // side ** c) % side + lo for c in range(d)], axis=1).astype(np.float64)


def _pow2(rng, count):
    return 2.0 ** rng.integers(-1, 3, count)


TIED_SEED = 7  # the first seed whose pattern leaves no row exactly ON a cut: with the seeds 0 .. 6 a group of three or four lattice
# points has a projection equal to its mid-range or to a neighbour's, and the last bits of the eigenvector decide the ids (the
# oracle's Jacobi routine and LAPACK's then disagree: tests/test_runsplit_cases.py)


def tied_pattern(d):
    rng = np.random.default_rng([2024, d, TIED_SEED])
    if d == 1:  # 24 distinct values, every one of them several times
        return rng.choice(np.arange(-8.0, 9.0), TIED_POINTS)[:, None], _pow2(rng, TIED_POINTS)
    P = np.zeros((TIED_POINTS, 3))
    P[:, 1:] = _distinct_points(rng, TIED_POINTS, -8, 8, 2)
    return P, _pow2(rng, TIED_POINTS)


def tied(d, forced):
    P, pw = tied_pattern(d)
    n = TIED_CLUSTERS * TIED_POINTS
    X, w = np.tile(P, (TIED_CLUSTERS, 1)), np.tile(pw, TIED_CLUSTERS)
    if d > 1:
        X[:, 0] += 64.0 * np.repeat(np.arange(TIED_CLUSTERS), TIED_POINTS)
    clusters = [list(range(q * TIED_POINTS + 1, (q + 1) * TIED_POINTS + 1)) for q in range(TIED_CLUSTERS)]
    lands = sorted({TIED_CLUSTERS * forced, TIED_CLUSTERS * forced + 1, 100, 400, n - 1, n})
    return Case(f"tied-d{d}-f{forced}", X, w, clusters, forced, lands)


def tied_cases():
    return [tied(d, f) for d in (3, 1) for f in TIED_FORCED]


BLOCKS_RANGE, BLOCKS_SEED = 64, 50
# The construction and the seed were chosen by the checks of tests/test_runsplit_cases.py.  With 150 points drawn freely from
# [-16, 16]^2 a seed can pass the Jacobi / LAPACK check (both routines produce the same bits on a degenerate group) and still
# give other ids with a third routine, the device's among them: under jittered eigenvectors (oracle.use_jittered_eig) no seed of
# 300 passed, nor of 400 in [-16, 16]^3.  The groups that decide it are {a, a, b} with a - b = (3, -3) and the like.  Keeping
# every pair of points off a common diagonal needs 150 distinct diagonals of either direction: [-64, 64]^2 is the smallest
# power-of-two range that has them with room for a rejection sampler.  Seed 50 is the first with n >= 350 that survives twelve
# jitter seeds at forced 1 and 4 under all four rules (0 and 25 leave a row on a cut of `diameter`, 1 and 26 give n < 350).


def _diagonal_free_points(rng, count, R):
    pts, seen, down, up = [], set(), set(), set()
    while len(pts) < count:
        x, y = (int(v) for v in rng.integers(-R, R + 1, 2))
        if (x, y) in seen or x - y in down or x + y in up:
            continue
        seen.add((x, y)), down.add(x - y), up.add(x + y)
        pts.append((x, y))
    return np.array(pts, dtype=np.float64)


def blocks(forced):
    rng = np.random.default_rng([1, BLOCKS_SEED])
    P = _diagonal_free_points(rng, 150, BLOCKS_RANGE)
    X = np.repeat(P, rng.integers(1, 5, 150), axis=0)
    X = X[rng.permutation(len(X))]
    n = len(X)
    clusters = [list(range(1, n // 2 + 1)), list(range(n // 2 + 1, n + 1))]
    return Case(f"blocks-f{forced}", X, np.full(n, 2.0), clusters, forced, ())


def distinct(forced):
    """the same kind of points without the repetitions (150 free points of [-16, 16]^2 fail the jitter check as `blocks` did: a
    group of three or four of them has a row on a cut or two components competing for the eigenvector's sign)"""
    rng = np.random.default_rng([3, 0])
    X = _diagonal_free_points(rng, 150, BLOCKS_RANGE)
    return Case(f"distinct-f{forced}", X, _pow2(rng, 150), [list(range(1, 151))], forced, ())


def error_cases():
    return [make(f) for make in (blocks, distinct) for f in (1, 4)]


def forced_groups(lengths, forced):
    """the number of groups the forced phase leaves: a cluster of at most `forced` rows becomes singletons, a longer one `forced`
    groups (src/landmarks.jl:282-313)"""
    return int(sum(min(k, max(forced, 1)) for k in lengths))


def forced_case(forced):
    rng = np.random.default_rng([5, forced])
    lengths = [1, 2, 3, forced, forced + 1, 40, 300]
    n = sum(lengths)
    X = _distinct_points(rng, n, -32, 32, 3)
    ids = rng.permutation(n) + 1
    clusters, at = [], 0
    for k in lengths:
        clusters.append([int(v) for v in ids[at:at + k]])
        at += k
    order = [5, 2, 6, 0, 4, 1, 3]  # the 300 rows in the middle, the single row behind them
    clusters = [clusters[i] for i in order]
    assert sorted(clusters) != clusters and any(sorted(c) != c for c in clusters)
    G = forced_groups(lengths, forced)
    return Case(f"forced-f{forced}", X, _pow2(rng, n), clusters, forced, (G - 3, G, G + 5))


def forced_cases():
    return [forced_case(f) for f in FORCED_VALUES]


def outcome(run, *args):
    """('ok', ids) or ('error', code) of a runsplit call, the oracle's or the library's"""
    try:
        return "ok", np.asarray(run(*args))
    except Exception as e:  # noqa: BLE001 -- OracleError.rc / CGEError.code
        code = getattr(e, "rc", None)
        if code is None:
            code = getattr(e, "code", None)
        if code is None:
            raise
        return "error", int(code)


def same_outcome(a, b):
    return a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "ok" else a[1] == b[1])


def oracle_outcome(orc, case, land, rule, lapack=False, jitter=None):
    """the oracle's outcome with its own Jacobi routine, with LAPACK's, or with LAPACK's and seeded jitter (oracle.use_jittered_eig)"""
    if jitter is not None:
        orc.use_jittered_eig(jitter)
    else:
        orc.use_lapack_eig(lapack)
    try:
        return outcome(orc.runsplit, case.X, case.w, case.clusters, land, case.forced, rule)
    finally:
        orc.use_lapack_eig(False)


def first_failing_land(orc, case, rule):
    """(land, code): the least `land` at which the oracle fails -- a failure at `land` is a failure at every greater one, since
    the pops of a run are a prefix of the pops of a longer one -- found by bisection between 1 and n + 1"""
    lo, hi = 1, case.n + 1
    assert oracle_outcome(orc, case, lo, rule)[0] == "ok"
    top = oracle_outcome(orc, case, hi, rule)
    assert top[0] == "error", (case, rule)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if oracle_outcome(orc, case, mid, rule)[0] == "ok":
            lo = mid
        else:
            hi = mid
    return hi, oracle_outcome(orc, case, hi, rule)[1]
