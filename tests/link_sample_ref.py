"""A plain reference of cge_link_sample (include/cge_hip.h) for tests/test_gpu_link_sample.py: numpy, nothing of the kernels.

    the sampled set   {(i, j) : u(i, j) < p(i, j)},  i < j (undirected) or every ordered i != j (directed)
    u(a, b)           (ctr_rand(seed, stream, a, b, 5) >> 11) * 2^-53, a and b the 0-based ids: the counter stream of
                      tests/local_score_ref.py, here vectorised in uint64 (wrapping arithmetic is what the stream is made of)

The GPU tests take p from the device's own cge_link_prob over all pairs and compare the sets with no tolerance; this module gives
them u, the set of a matrix of p, and the inputs.  tests/test_link_sample_ref.py holds u against the scalar stream and the inputs
to the conditions the GPU tests rely on.
"""
import numpy as np

import link_ref as lr

WHICH = 5
_M = np.uint64


def _sm64(x):
    x = x + _M(0x9E3779B97F4A7C15)
    x = (x ^ (x >> _M(30))) * _M(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> _M(27))) * _M(0x94D049BB133111EB)
    return x ^ (x >> _M(31))


def rand64(seed, stream, a, b, which=WHICH):
    """ctr_rand(seed, stream, a, b, which) for arrays a, b (broadcast), as uint64."""
    a, b = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _sm64(_M(seed & 0xFFFFFFFFFFFFFFFF) ^ _M(0x6A09E667F3BCC909))
        h = _sm64(h ^ (_M(stream & 0xFFFFFFFFFFFFFFFF) * _M(0xD1342543DE82EF95) + _M(1)))
        h = _sm64(h ^ (a * _M(0x2545F4914F6CDD1D) + _M(2)))
        h = _sm64(h ^ (b * _M(0x9E6C63D0676A9A99) + _M(3)))
        return _sm64(h ^ _M(which + 4))


def uniform(seed, stream, a, b):
    """u(a, b) in [0, 1): the top 53 bits of the draw, exact in fp64."""
    return (rand64(seed, stream, a, b) >> _M(11)).astype(np.float64) * 2.0 ** -53


def all_pairs(n, directed):
    """The pairs a draw is made over, 0-based, sorted by (i, j)."""
    if directed:
        i, j = np.divmod(np.arange(n * n, dtype=np.int64), n)
        keep = i != j
        return i[keep], j[keep]
    i, j = np.triu_indices(n, 1)
    return i.astype(np.int64), j.astype(np.int64)


def uniform_matrix(seed, stream, n):
    a, b = np.divmod(np.arange(n * n, dtype=np.int64), n)
    return uniform(seed, stream, a, b).reshape(n, n)


def sampled(i, j, p, u):
    """The sampled set of the pairs (i, j) (sorted by (i, j)) with values p and uniforms u: (i, j, p) of the edges."""
    e = np.asarray(u) < np.asarray(p)
    return i[e], j[e], np.asarray(p)[e]


# ---- the inputs the GPU tests and their CPU conditions share ---------------------------------------------------------------------
# (n, d, directed); the rows of (600, 40) carry a common offset of 1e6 (the Gram formula's cancellation)
SHAPES = [(1, 3, False), (2, 1, False), (2, 1, True), (127, 17, False), (128, 40, True), (129, 1, False), (257, 130, False),
          (257, 16, True), (600, 40, False), (1000, 17, False), (1000, 16, True)]
ALPHA = 2.25
MEAN_P = 0.05


def shape_id(s):
    return "n%d-d%d-%s" % (s[0], s[1], "dir" if s[2] else "und")


_CASES = {}


def shape_case(n, d, directed):
    """Points, hi = the diameter, lognormal factors scaled so that the mean p over the pairs is near MEAN_P; then one vertex with
    factor 1e3 (its pairs have p > 1) and three with factor 0.  A resident graph is needed by the model and plays no part."""
    key = (n, d, directed)
    if key in _CASES:
        return _CASES[key]
    seed = 100 + n + d + (1 if directed else 0)
    rng = np.random.default_rng(seed)
    X = lr.points(n, d, seed, offset=1e6 if (n, d) == (600, 40) else 0.0)
    hi = max(lr.diameter(X)[0], 1.0) * (1.0 if n >= 127 else 2.0)  # (two points are their own diameter: p would be 0)
    fo = np.exp(0.5 * rng.standard_normal(n))
    fi = np.exp(0.5 * rng.standard_normal(n)) if directed else None
    i, j = all_pairs(n, directed)
    if n >= 127:
        mean = float(np.mean(lr.prob(X, hi, ALPHA, fo, fi, i, j)))
        s = np.sqrt(MEAN_P / mean)
        fo = fo * s
        fi = None if fi is None else fi * s
    if n >= 127:
        special = rng.permutation(n)[:4]
        for f in (fo, fi):
            if f is not None:
                f[special[0]] = 1e3
                f[special[1:]] = 0.0
    edges = lr.random_edges(n, 4 * n, seed, directed) if n > 1 else np.zeros((1, 2), np.int64)
    c = dict(X=X, hi=hi, alpha=ALPHA, fo=fo, fi=fi, directed=directed, edges=edges, n=n)
    _CASES[key] = c
    return c


def threshold_case(n, directed, clamped, seed=7):
    """n points in 8 dimensions for the hook's tests: every factor positive but three; clamped: hi is half the diameter."""
    rng = np.random.default_rng(seed + n + 2 * directed + 4 * clamped)
    X = lr.points(n, 8, seed + n)
    hi = lr.diameter(X)[0] * (0.5 if clamped else 1.0)
    fo = 0.4 * np.exp(0.5 * rng.standard_normal(n))
    fi = 0.4 * np.exp(0.5 * rng.standard_normal(n)) if directed else None
    for f in (fo, fi):
        if f is not None:
            f[[5, 150, 299 % n]] = 0.0
    return dict(X=X, hi=hi, alpha=ALPHA, fo=fo, fi=fi, directed=directed, edges=lr.random_edges(n, 4 * n, seed, directed), n=n)
