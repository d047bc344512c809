"""Reference, a-priori bound and named inputs of cge_link_triangles (no GPU, numpy only).

Model side.  q(i, j) = min(p(i, j), 1), q(i, i) = 0, Q the symmetric matrix of the q (fp64 numbers: EXACT by definition).  Then

    t_i = 1/2 sum_j Q_ij (Q Q)_ij = sum over the pairs j < k of q_ij q_jk q_ik        (expected triangles through i)
    w_i = sum over the pairs j < k of q_ij q_ik                                      (expected wedges centred at i)

in numpy.longdouble: by the triple loop for tiny n (`expected_loops`), by the matrix form (`expected`) otherwise; tests/
test_link_triangles_ref.py holds the two to each other.  `model_q` builds Q from tests/link_ref.py's p rounded to fp64 -- what
cge_link_prob returns up to link_ref.BOUND; the GPU tests build the reference from the device's OWN Q (fetched through the testing
hook and held to cge_link_prob bit for bit there), because the contract is stated against Q's entries.

The bound (include/cge_hip.h, derived in DESIGN.md section 4.17):  |got - exact| <= (n + 8) 2^-52 exact + n^2 2^-1073.

Graph side.  The edge list as a simple undirected graph; triangles through v and wedges k_v (k_v - 1) / 2 by brute force over
vertex triples (`observed_loops`, tiny n) and from the 0/1 adjacency matrix (`observed`: diag(A^3) / 2 in float64, exact while the
counts stay below 2^53); the same CPU test holds the two to each other."""
import itertools

import numpy as np

import link_ref as lr

LD = np.longdouble


def bound(n, exact):
    """The a-priori bound of an output whose exact value (long double) is `exact`, as float64."""
    return ((n + 8) * LD(2.0) ** -52 * np.asarray(exact, LD) + LD(n) * LD(n) * LD(2.0) ** -1073).astype(np.float64)


def model_q(c):
    """Q (n, n) float64 of an undirected case: link_ref.prob rounded to fp64, clamped at 1, zero diagonal."""
    n = len(c["X"])
    i, j = np.divmod(np.arange(n * n, dtype=np.int64), n)
    p = lr.prob(c["X"], c["hi"], c["alpha"], c["fo"], None, i, j).astype(np.float64).reshape(n, n)
    Q = np.minimum(p, 1.0)
    np.fill_diagonal(Q, 0.0)
    return Q


def expected(Q):
    """(t, w) long double (n,) each, the matrix form: t = rowsum(Q o (Q Q)) / 2, w_i = sum_k q_ik (sum_{j<k} q_ij)."""
    Ql = np.asarray(Q, LD)
    t = (Ql * (Ql @ Ql)).sum(1) / LD(2)
    before = np.zeros_like(Ql)
    before[:, 1:] = np.cumsum(Ql, axis=1)[:, :-1]
    return t, (Ql * before).sum(1)


def expected_loops(Q):
    """The same by the triple loop over i and the pairs j < k (n <= 40)."""
    Ql = np.asarray(Q, LD)
    n = len(Ql)
    t, w = np.zeros(n, LD), np.zeros(n, LD)
    for i in range(n):
        for j in range(n):
            for k in range(j + 1, n):
                w[i] += Ql[i, j] * Ql[i, k]
                t[i] += Ql[i, j] * Ql[j, k] * Ql[i, k]
    return t, w


def adjacency(edges, n):
    """The distinct-neighbour sets of 0-based rows: either orientation, repeats once, loops dropped."""
    nb = [set() for _ in range(n)]
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2):
        if a != b:
            nb[int(a)].add(int(b))
            nb[int(b)].add(int(a))
    return nb


def observed_loops(edges, n):
    """(tri, wed) int64 by brute force over the vertex triples."""
    nb = adjacency(edges, n)
    tri = np.zeros(n, np.int64)
    for a, b, c in itertools.combinations(range(n), 3):
        if b in nb[a] and c in nb[a] and c in nb[b]:
            tri[[a, b, c]] += 1
    k = np.array([len(s) for s in nb], np.int64)
    return tri, k * (k - 1) // 2


def observed(edges, n):
    """(tri, wed) int64 from the 0/1 adjacency matrix: tri = diag(A^3) / 2, in float64 (exact: every count is far below 2^53)."""
    A = np.zeros((n, n))
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    tri = ((A @ A) * A).sum(1) / 2.0
    k = A.sum(1).astype(np.int64)
    assert (tri == np.round(tri)).all() and tri.max(initial=0) < 2.0 ** 52
    return tri.astype(np.int64), k * (k - 1) // 2


# ---- the named graphs ---------------------------------------------------------------------------------------------------------------
def _clique(ids):
    return [(a, b) for a, b in itertools.combinations(ids, 2)]


def graphs():
    """name -> (n, edges (m, 2) 0-based).  The known-answer graphs of the issue, then the shapes the kernels can go wrong at."""
    g = {}
    g["k9"] = (9, _clique(range(9)))                                           # 28 triangles per vertex
    g["star"] = (8, [(0, v) for v in range(1, 8)])                             # none
    g["two_k5_sharing_a_vertex"] = (9, _clique(range(5)) + _clique(range(4, 9)))  # 6 per vertex, 12 at the shared one
    g["cycle5"] = (5, [(v, (v + 1) % 5) for v in range(5)])                    # none; one wedge per vertex
    base = _clique(range(4)) + [(4, 5), (5, 6), (6, 4), (0, 4)]
    g["multigraph"] = (8, base + [(b, a) for a, b in base] + base[:5] + [(1, 1), (7, 7), (4, 4)])
    g["multigraph_simple"] = (8, base)
    rng = np.random.default_rng(31)
    e = rng.integers(0, 300, (3000, 2))
    e[:40, 1] = e[:40, 0]              # loops
    e[40:400] = e[400:760]             # repeated rows
    e[760:900] = e[900:1040][:, ::-1]  # ... and their other orientation
    g["random_multigraph_n300"] = (300, e)
    rng = np.random.default_rng(32)
    e = rng.integers(0, 40, (120, 2))
    e = e[(e % 5 != 0).all(1)]  # vertices 0, 5, 10, ... are isolated
    g["isolated_vertices"] = (40, e)
    # n = 1200: vertex 0 has 1100 distinct neighbours, vertex 1 has 70, and a clique of 90 (ids 1100 .. 1189) whose ORIENTED
    # lists run up to 89 entries -- the orientation by degree keeps a hub's own list short, a clique's not -- plus random rows
    rng = np.random.default_rng(33)
    e = [(0, v) for v in range(2, 1102)] + [(1, v) for v in range(500, 570)] + _clique(range(1100, 1190))
    e += [tuple(r) for r in rng.integers(0, 1200, (3000, 2))]
    g["hubs_and_clique_n1200"] = (1200, e)
    return {k: (n, np.asarray(e, np.int64).reshape(-1, 2)) for k, (n, e) in g.items()}


KNOWN = {"k9": (np.full(9, 28), np.full(9, 28)), "star": (np.zeros(8, np.int64), np.array([21] + [0] * 7)),
         "two_k5_sharing_a_vertex": (np.array([6, 6, 6, 6, 12, 6, 6, 6, 6]), np.array([6, 6, 6, 6, 28, 6, 6, 6, 6])),
         "cycle5": (np.zeros(5, np.int64), np.ones(5, np.int64))}


# ---- the named models ---------------------------------------------------------------------------------------------------------------
def _model(n, d, alpha, seed, scale=0.5, hi_factor=1.0, X=None, fo=None):
    rng = np.random.default_rng(seed)
    X = lr.points(n, d, seed) if X is None else X
    fo = scale * np.exp(0.5 * rng.standard_normal(n)) if fo is None else np.asarray(fo, np.float64)
    edges = lr.random_edges(n, 4 * n, seed, False)
    return dict(X=np.asarray(X, np.float64), hi=float(max(lr.diameter(X)[0], 1e-300) * hi_factor), alpha=float(alpha), fo=fo, edges=edges)


def models():
    """name -> undirected case (X, hi, alpha, fo, edges).  n on both sides of the 64- and 128-tiles (5, 127, 128, 129, 257, 385:
    one, two and three tile rows, so that off-diagonal tiles feed both their row and their column block), d = 3, 8, 130, alpha =
    0.25, 1, 6.25."""
    c = {}
    c["n5_d3"] = _model(5, 3, 1.0, 41)
    c["n127_d8"] = _model(127, 8, 0.25, 42)
    c["n128_d130"] = _model(128, 130, 6.25, 43, scale=3.0)
    c["n129_d3"] = _model(129, 3, 6.25, 44)
    c["n257_d8"] = _model(257, 8, 1.0, 45)
    c["n385_d130"] = _model(385, 130, 0.25, 46, scale=0.3)
    c["n257_saturated"] = _model(257, 3, 1.0, 47, scale=4.0)  # many pairs with p > 1
    z = _model(129, 8, 1.0, 48)
    z["fo"][[0, 5, 64, 128]] = 0.0
    c["n129_zero_factors"] = z
    c["n257_small_hi"] = _model(257, 3, 0.25, 49, hi_factor=0.5)  # entries that are exactly 0
    X = lr.points(129, 8, 50)
    X[60:70] = X[0]
    c["n129_repeated_rows"] = _model(129, 8, 6.25, 50, X=X)
    # every factor equal on a ring: all rows alike up to rotation, so a mis-addressed tile still gives a plausible TOTAL
    ang = 2.0 * np.pi * np.arange(300) / 300.0
    c["n300_equal_factors"] = _model(300, 3, 1.0, 51, X=np.stack([np.cos(ang), np.sin(ang), 0.0 * ang], 1), fo=np.full(300, 0.7))
    h = _model(385, 3, 1.0, 52, scale=0.2)
    h["fo"][200] = 40.0  # one heavy vertex
    c["n385_heavy_vertex"] = h
    return c


def all_ones_model(n):
    """Every q = 1: every factor 2, every point the same (base 1)."""
    return dict(X=np.zeros((n, 3)), hi=1.0, alpha=1.0, fo=np.full(n, 2.0), edges=np.array([[0, 1]], np.int64))


# ---- against draws --------------------------------------------------------------------------------------------------------------------
DRAW_N, DRAW_DRAWS, DRAW_SEED = 120, 64, 2024


def draw_model():
    return _model(DRAW_N, 3, 1.0, 60, scale=0.55)


def draw_condition(Q, totals_tri, totals_wed):
    """The issue's condition on `DRAW_DRAWS` draws: (z_tri, z_wed) = (mean total - expectation) / standard error, the totals
    being the draws' triangle counts (sum tri / 3) and wedge counts, the standard errors estimated from the same draws."""
    t, w = expected(Q)
    out = []
    for tot, ex in ((np.asarray(totals_tri, np.float64), float(t.sum() / 3)), (np.asarray(totals_wed, np.float64), float(w.sum()))):
        se = tot.std(ddof=1) / np.sqrt(len(tot))
        out.append((tot.mean() - ex) / se)
    return tuple(out)


def cpu_draws(Q):
    """The draws cge_link_sample makes on the streams 0 .. DRAW_DRAWS - 1 of DRAW_SEED, reproduced with tests/link_sample_ref.py:
    per draw (triangles, wedges) of the sampled graph by `observed`."""
    import link_sample_ref as sr

    n = len(Q)
    i, j = np.triu_indices(n, 1)
    tri, wed = [], []
    for s in range(DRAW_DRAWS):
        u = sr.uniform_matrix(DRAW_SEED, s, n)[i, j]
        keep = u < Q[i, j]
        t, w = observed(np.stack([i[keep], j[keep]], 1), n)
        tri.append(t.sum() // 3)
        wed.append(w.sum())
    return np.array(tri), np.array(wed)
