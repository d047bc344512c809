"""A plain reference of the link model (cge_link_prob / cge_link_topk, include/cge_hip.h) for tests/test_gpu_link.py: numpy and
long double, nothing of the kernels.

    p(i, j) = f_out[i] * f_in[j] * max(0, 1 - dist(i, j) / hi) ^ alpha

  dist          `local_score_ref.dist`: fp64, one rounding per operation, ascending k (src/auxilary.jl:14-20);
  the base      x = d / hi and 1 - x in fp64, clamped at 0 -- the device takes the same four operations (a subtraction, a product,
                an addition per feature; a correctly rounded root and quotient), so the base has the device's bits;
  the value     the power and the two products in long double (64-bit significand);
  top-k         brute force per query under the total order (p descending, j ascending) with the exclusion rules of the header.

The bound between a device p and this reference's, derived rather than chosen (u = 2^-53, one rounding to nearest):
  * the base is bit-identical (above), so the power's argument is exact on both sides;
  * the device power is within 2 ulp of the true one in either form: the stored-logarithm form is pinned within one ulp of glibc's
    pow (tests/test_gpu_parity.py::test_pow_from_stored_logarithm_is_within_one_ulp), itself below one ulp; the library pow is
    within one ulp (the premise of tests/test_gpu_local_score.py's tallies) -- one bound, the larger, serves both.  An ulp is at
    most 2 u of the value: 4 u;
  * the two products round once each: 2 u;
  * this reference's own three operations in long double: 3 x 2^-64; the second-order terms of the product of the three factors
    (15 u^2) are far below one more 2^-64.  The comparison itself is made in long double.
  BOUND = 6 u + 4 x 2^-64 (6.7e-16), relative to the value; a p of exactly 0 (base 0, or a zero factor) is 0 on both sides.
"""
import numpy as np

from local_score_ref import dist

LD = np.longdouble
U = 2.0 ** -53
BOUND = 6 * U + 4 * 2.0 ** -64


def base(X, i, j, hi):
    """max(0, 1 - dist / hi) in fp64, the device's bits."""
    b = 1.0 - dist(X, np.asarray(i), np.asarray(j), hi)
    return np.where(b < 0.0, 0.0, b)


def prob(X, hi, alpha, f_out, f_in, i, j):
    """p of the 0-based pairs (i[q], j[q]) in long double."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    fo, fi = np.asarray(f_out, LD), np.asarray(f_out if f_in is None else f_in, LD)
    return (fo[i] * fi[j]) * np.asarray(base(X, i, j, hi), LD) ** LD(alpha)


def neighbours(edges, n, directed):
    """Per vertex the set of vertices a resident edge excludes: either orientation when undirected, i -> j alone when directed.
    `edges`: 0-based (m, 2); repeated rows and self loops change nothing (a self loop excludes what is excluded anyway)."""
    out = [set() for _ in range(n)]
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2):
        out[a].add(int(b))
        if not directed:
            out[b].add(int(a))
    return out


def admissible(i, n, nbrs, exclude):
    """The candidates of query i, ascending."""
    drop = {i} | (nbrs[i] if exclude else set())
    return np.array([j for j in range(n) if j not in drop], np.int64)


def topk(X, hi, alpha, f_out, f_in, queries, k, edges=None, directed=False, exclude=True):
    """Per query (0-based, repeats allowed): (j (Q, k) 0-based, p (Q, k) long double, count (Q,), values) -- the k admissible
    candidates of largest p, ties to the smaller j, by insertion into a running list; unused slots hold -1 / 0.  values[q] =
    (candidates, their p) for the margin checks of the GPU test."""
    n = len(X)
    nbrs = neighbours(edges if edges is not None else np.zeros((0, 2), np.int64), n, directed)
    Q = len(queries)
    J, P, cnt, vals = -np.ones((Q, k), np.int64), np.zeros((Q, k), LD), np.zeros(Q, np.int64), []
    for q, i in enumerate(np.asarray(queries, np.int64)):
        cand = admissible(int(i), n, nbrs, exclude)
        p = prob(X, hi, alpha, f_out, f_in, np.full(len(cand), i), cand) if len(cand) else np.zeros(0, LD)
        vals.append((cand, p))
        best = []  # (p, j), kept sorted by (p descending, j ascending)
        for pj, j in zip(p, cand):
            pos = len(best)
            while pos > 0 and (best[pos - 1][0] < pj or (best[pos - 1][0] == pj and best[pos - 1][1] > j)):
                pos -= 1
            if pos < k:
                best.insert(pos, (pj, int(j)))
                del best[k:]
        cnt[q] = len(best)
        for t, (pj, j) in enumerate(best):
            J[q, t], P[q, t] = j, pj
    return J, P, cnt, vals


def topk_by_sort(cand, p, k):
    """The same list from an independent full sort of one query's candidates: (j, p)."""
    order = np.lexsort((cand, -np.asarray(p, LD)))[:k]
    return cand[order], p[order]


def kth_gap(p_sorted_desc, k):
    """Relative gap between the k-th and (k+1)-th values of a descending list (inf when there is no (k+1)-th)."""
    if len(p_sorted_desc) <= k:
        return np.inf
    a, b = p_sorted_desc[k - 1], p_sorted_desc[k]
    return float((a - b) / a) if a > 0 else 0.0


# ---- the inputs the GPU tests and their CPU conditions share ---------------------------------------------------------------------
def points(n, d, seed, offset=0.0):
    return np.random.default_rng(seed).standard_normal((n, d)) + offset


def diameter(X):
    """The point-set diameter in dist()'s arithmetic and a pair attaining it (the smallest (i, j))."""
    n = len(X)
    ii, jj = np.triu_indices(n, 1)
    if len(ii) == 0:
        return 0.0, 0, 0
    dd = dist(X, ii, jj, 1.0)
    a = int(np.argmax(dd))
    return float(dd[a]), int(ii[a]), int(jj[a])


def random_edges(n, m, seed, directed):
    """m random rows (0-based), among them repeated rows, both orientations of some pairs and a few self loops."""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, (m, 2))
    if m >= 8:
        e[1] = e[0]            # a repeated edge
        e[2] = e[0][::-1]      # ... and its other orientation
        e[3] = (e[3][0], e[3][0])  # a self loop
    return e.astype(np.int64)


# the shapes of tests/test_gpu_link.py::test_topk_shapes: every n, d, Q and k of the issue occurs, on both sides of the 128-row and
# 128-candidate tiles, with and without exclusion, directed and not: (n, d, Q, k, directed, exclude, seed)
TOPK_SHAPES = [
    (2, 1, 1, 1, False, False, 1),
    (2, 16, 3, 7, False, True, 2),
    (127, 17, 128, 32, False, True, 3),
    (128, 40, 129, 33, True, True, 4),
    (129, 1, 300, 64, False, False, 5),
    (257, 16, 3, 64, True, False, 6),
    (257, 17, 300, 7, False, True, 7),
    (1000, 40, 1, 1, False, True, 8),
    (1000, 16, 128, 32, True, True, 9),
    (1000, 17, 129, 33, False, False, 10),
    (1000, 1, 300, 7, True, True, 11),
    (129, 40, 128, 64, True, True, 12),
]


def shape_case(n, d, Q, k, directed, exclude, seed):
    """One input of TOPK_SHAPES: points, lognormal factors, hi = the diameter, queries (Q = 300: with repeats), random edges."""
    rng = np.random.default_rng(1000 + seed)
    X = points(n, d, seed)
    hi = max(diameter(X)[0], 1.0)
    fo = np.exp(0.5 * rng.standard_normal(n))
    fi = np.exp(0.5 * rng.standard_normal(n)) if directed else None
    queries = rng.integers(0, n, Q) if Q == 300 else rng.permutation(max(n, Q))[:Q] % n
    edges = random_edges(n, 4 * n, seed, directed)
    return dict(X=X, hi=hi, alpha=2.25, fo=fo, fi=fi, queries=queries.astype(np.int64), k=k, edges=edges, directed=directed,
                exclude=exclude)


def _case(X, hi, alpha, fo, fi, queries, k, edges, directed, exclude, exact=False):
    return dict(X=np.asarray(X, np.float64), hi=float(hi), alpha=float(alpha), fo=np.asarray(fo, np.float64),
                fi=None if fi is None else np.asarray(fi, np.float64), queries=np.asarray(queries, np.int64), k=int(k),
                edges=np.asarray(edges, np.int64).reshape(-1, 2), directed=bool(directed), exclude=bool(exclude), exact=bool(exact))


# the cases of tests/test_gpu_link.py::test_topk_cases.  exact = the returned ids are compared with this reference's one by one;
# tests/test_link_ref.py holds the condition that allows it: every two neighbours among the first k + 1 reference values of a
# query are equal (a tie by construction: duplicated rows with equal factors give the device equal bits too) or more than
# 2 BOUND apart.
def stress_cases():
    c = {}
    rng = np.random.default_rng(77)
    # counts and empty slots: k >= n; a query adjacent to every vertex; a star's hub and a leaf; exclusion off and on
    X5 = points(5, 3, 21)
    star = [(0, 1), (0, 2), (3, 0), (0, 4)]
    for ex in (False, True):
        c[f"k_beyond_n_exclude{int(ex)}"] = _case(X5, diameter(X5)[0], 1.5, [1.0, 2.0, 0.5, 1.5, 3.0], None, [0, 1, 4, 0], 7, star,
                                                  False, ex, exact=True)
    # directed: j -> i exists and i -> j does not (query 1: 0 -> 1 does not exclude 0; query 0: 0 -> 1 excludes 1)
    c["directed_one_way"] = _case(X5, diameter(X5)[0], 1.5, [1.0, 2.0, 0.5, 1.5, 3.0], [2.0, 1.0, 1.0, 0.25, 1.0], [0, 1, 2, 3, 4], 4,
                                  [(0, 1), (2, 3), (3, 2), (4, 0)], True, True, exact=True)
    # repeated edges and self loops change nothing
    c["repeats_and_loops"] = _case(X5, diameter(X5)[0], 1.5, [1.0, 2.0, 0.5, 1.5, 3.0], None, [0, 1, 2, 3, 4], 4,
                                   [(0, 1), (1, 0), (0, 1), (2, 2), (3, 3), (3, 4), (3, 4)], False, True, exact=True)
    # duplicated rows with equal factors: exact ties, the smaller j first
    X = points(300, 8, 22)
    X[100:200] = X[0:100]
    fo = np.exp(0.5 * rng.standard_normal(300))
    fo[100:200] = fo[0:100]
    c["duplicated_rows"] = _case(X, diameter(X)[0], 2.25, fo, None, np.arange(0, 300, 7), 33, [(0, 1)], False, False, exact=True)
    # all factors equal: the order is the nearest-neighbour order
    X = points(257, 17, 23)
    c["equal_factors"] = _case(X, diameter(X)[0], 3.0, np.ones(257), None, np.arange(0, 257, 5), 32, [(0, 1)], False, False,
                               exact=True)
    # one far vertex whose factor outranks every near one: a filter that looks at distance alone loses it
    X = points(400, 16, 24)
    X[399] = 0.0
    X[399, 0] = 0.9 * diameter(X[:399])[0]
    fi = np.ones(400)
    fi[399] = 1e9
    c["far_heavy_vertex"] = _case(X, diameter(X)[0], 4.0, fi, None, np.arange(0, 399, 9), 7, [(0, 1)], False, False)
    # a zero factor: as a candidate it ranks last, as a query every p is 0 and the smallest ids win
    X = points(200, 16, 25)
    fo = np.exp(0.5 * rng.standard_normal(200))
    fo[[3, 50, 130]] = 0.0
    c["zero_factor"] = _case(X, diameter(X)[0], 2.0, fo, None, [3, 4, 50, 199], 64, random_edges(200, 400, 25, False), False, True)
    # rows with a large common offset: the Gram formula's cancellation; the filter must stay conservative
    X = points(600, 40, 26, offset=1e6)
    c["common_offset"] = _case(X, diameter(X)[0], 2.25, np.exp(0.5 * rng.standard_normal(600)), None, np.arange(0, 600, 4), 32,
                               random_edges(600, 2400, 26, False), False, True)
    # candidates that arrive in ascending score: every tile inserts
    X = np.arange(1000, dtype=np.float64).reshape(-1, 1)
    c["ascending_scores"] = _case(X, 999.0, 2.0, np.ones(1000), None, [999, 998, 0, 500], 33, [(0, 1)], False, False,
                                  exact=True)
    # ... and in descending score: the first candidate tile (ids 0 .. 127, a unit grid) holds every query's best 33, every later
    # tile lies beyond a gap.  A workgroup that walks tile 0 and then others has a k-th value more than twice what they hold at
    # best (tests/test_link_ref.py), so its filter must reject them: the thresholds are seen to bite
    X = np.arange(1000, dtype=np.float64).reshape(-1, 1)
    X[128:] += 500.0
    c["descending_scores"] = _case(X, 1499.0, 2.0, np.ones(1000), None, [0, 127, 64, 31], 33, [(0, 1)], False, False, exact=True)
    # the same grid, and in the candidate tiles 2, 4 and 6 one vertex per query that beats the query's k-th value so far by a
    # hair: its squared distance is 1 - 2e-4 of the k-th's, 1 - 4e-4, 1 - 6e-4.  A workgroup that has walked tile 0 must let each
    # of them through; a threshold radius that is 1e-3 too tight (squared) drops them, and the list is wrong in its last entry
    X = np.arange(1000, dtype=np.float64).reshape(-1, 1)
    X[128:] += 700.0
    for t, v in enumerate(NEAR_THRESHOLD_IDS):
        X[v, 0] = -33.0 * (1.0 - 1e-4) ** (t + 1)            # query 0: its 33rd of tile 0 is vertex 33, at distance 33
        X[v + 1, 0] = 127.0 + 33.0 * (1.0 - 1e-4) ** (t + 1)  # query 127: vertex 94
    c["near_threshold"] = _case(X, float(X.max() - X.min()), 2.0, np.ones(1000), None, [0, 127], 33, [(0, 1)], False, False,
                                exact=True)
    return c


NEAR_THRESHOLD_IDS = (300, 600, 800)  # in the candidate tiles 2, 4, 6 (with the next id: the second query's)


def merge_case(n, seed):
    """The input of tests/test_gpu_link.py's merge tests: Q = 2 queries, k = 64, d = 3, hi = twice the largest distance from the
    mean (at least the diameter, without its O(n^2) search), lognormal factors; the vertices of the last 129 ids carry a factor 3,
    so that the candidate slices with the highest numbers have entries in both lists (checked where it is used)."""
    rng = np.random.default_rng(seed)
    X = points(n, 3, seed)
    hi = 2.0 * float(np.sqrt(((X - X.mean(axis=0)) ** 2).sum(axis=1)).max())
    fo = np.exp(0.5 * rng.standard_normal(n))
    fo[-129:] *= 3.0
    return _case(X, hi, 2.25, fo, None, [n - 1, 5], 64, [(0, 1)], False, False)
