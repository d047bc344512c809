"""Seeded symmetric test matrices for the principal-eigenvector solvers (host: cge_host_eig_top; device: cge_group_eig), and
the criterion they are judged by.  The families are the matrices real embeddings produce and random Wishart matrices never
do: clustered and repeated top eigenvalues, graded spectra, rank-deficient covariances, near-isotropic clouds, diagonal and
splitting tridiagonal matrices, entries scaled far from 1.  One matrix per family and width.

Criterion (no vector comparison across a tiny gap).  U = eps sqrt(d) ||A||_2, v the returned vector:
  * | ||v|| - 1 | <= 4 eps sqrt(d); the component of largest magnitude is positive, or within 2 ulp of one that is;
  * the residual ||A v - (v'Av) v|| and the deficit lambda_max - v'Av are each at most 8 max(U, what numpy.linalg.eigh's own
    top vector scores on the same matrix); lambda_max is LAPACK's.  The limit comes from the reference, never from the solver
    under test.  The factor 8 covers approximate reciprocals, one inverse iteration fewer and another update order; a structural
    error (a missed reflector, a wrong column slot, the silent e_1 fallback) sits many orders above it.
Residual and deficit are evaluated in long double, so the evaluation's own rounding stays below U."""
import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble


def _orth(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def _sym(a):
    return (a + a.T) / 2


def _from_spectrum(rng, lam):
    q = _orth(rng, len(lam))
    return _sym((q * np.asarray(lam)) @ q.T)


def _rest(rng, d, top):
    """`top` (the leading eigenvalues, as many as fit) over a bulk in 0.1 .. 0.9"""
    top = list(top)[:d]
    return np.array(top + list(rng.uniform(0.1, 0.9, d - len(top))))


def _wilkinson(n):
    a = np.diag(np.abs(np.arange(n) - (n - 1) / 2.0))
    i = np.arange(n - 1)
    a[i, i + 1] = a[i + 1, i] = 1.0
    return a


def _glued_wilkinson(d, glue=1e-8, block=21):
    b = min(block, d)
    a = np.diag(np.abs((np.arange(d) % b) - (b - 1) / 2.0))
    i = np.arange(d - 1)
    off = np.where((i + 1) % b == 0, glue, 1.0)
    a[i, i + 1] = a[i + 1, i] = off
    return a


def _wishart(rng, d, k=None):
    k = k or 2 * d + 3
    y = rng.standard_normal((k, d)) * rng.uniform(0.2, 3.0, d)
    return y.T @ y


def _cov(x, w=None):
    w = np.ones(len(x)) if w is None else w
    mu = (x * w[:, None]).sum(0) / w.sum()
    y = (x - mu) * np.sqrt(w)[:, None]
    return y.T @ y


def _two_blocks(rng, d):
    h = d // 2
    b = _wishart(rng, h) if h else np.zeros((0, 0))
    a = np.zeros((d, d))
    a[:h, :h] = b
    a[h:2 * h, h:2 * h] = b
    if d % 2:
        a[-1, -1] = 0.25 * (b.max() if h else 1.0)
    return a


def _offdiag_tiny(rng, d):
    a = np.full((d, d), 1e-20)
    a[np.arange(d), np.arange(d)] = rng.uniform(0.5, 2.0, d)
    return a


def _diag_permuted(rng, d):
    p = rng.permutation(np.arange(1.0, d + 1))
    if p[-1] == d:  # the largest entry is not the last one
        p[0], p[-1] = p[-1], p[0]
    return np.diag(p)


def _scaled(a, s):
    return a / np.abs(a).max() * s


FAMILIES = {
    # ---- spectrum families: Q diag(lambda) Q' with a random orthogonal Q
    "gap_1e-10": lambda rng, d: _from_spectrum(rng, _rest(rng, d, [1.0, 1.0 - 1e-10])),
    "gap_1e-14": lambda rng, d: _from_spectrum(rng, _rest(rng, d, [1.0, 1.0 - 1e-14])),
    "top_three_equal": lambda rng, d: _from_spectrum(rng, _rest(rng, d, [1.0, 1.0, 1.0])),
    "scaled_identity": lambda rng, d: 3.7 * np.eye(d),
    "rank_1": lambda rng, d: (lambda u: 2.5 * np.outer(u, u) / (u @ u))(rng.standard_normal(d)),
    "graded_1e16": lambda rng, d: _from_spectrum(rng, 10.0 ** (-16.0 * np.arange(d) / max(d - 1, 1))),
    "graded_1e30": lambda rng, d: _from_spectrum(rng, 10.0 ** (-30.0 * np.arange(d) / max(d - 1, 1))),
    # ---- structured families
    "diag_descending": lambda rng, d: np.diag(np.arange(d, 0, -1.0)),
    "diag_permuted": lambda rng, d: _diag_permuted(rng, d),
    "wilkinson": lambda rng, d: _wilkinson(d),
    "glued_wilkinson": lambda rng, d: _glued_wilkinson(d),
    "glued_wilkinson_dense": lambda rng, d: (lambda q: _sym(q @ _glued_wilkinson(d) @ q.T))(_orth(rng, d)),
    "two_equal_blocks": _two_blocks,
    "offdiag_1e-20": _offdiag_tiny,
    "all_ones": lambda rng, d: np.ones((d, d)),
    # ---- covariances and scales
    "cov_2_points": lambda rng, d: _cov(rng.standard_normal((2, d)), np.array([3.0, 5.0])),
    "cov_d/4_points": lambda rng, d: _cov(rng.standard_normal((max(3, d // 4), d)), rng.integers(1, 41, max(3, d // 4)).astype(float)),
    "cov_isotropic_50d": lambda rng, d: _cov(rng.standard_normal((50 * d, d))),
    "cov_offset_cloud": lambda rng, d: _cov(1e3 + 1e-3 * rng.standard_normal((3 * d + 5, d))),
    "scale_1e+150": lambda rng, d: _scaled(_wishart(rng, d), 1e150),
    "scale_1e-150": lambda rng, d: _scaled(_wishart(rng, d), 1e-150),
}


def family_matrix(name, d, seed=0):
    """The matrix of family `name` at width d: symmetric to the bit, C-contiguous fp64."""
    rng = np.random.default_rng([seed, d, sorted(FAMILIES).index(name)])
    a = np.ascontiguousarray(FAMILIES[name](rng, d), dtype=np.float64)
    assert a.shape == (d, d) and np.array_equal(a, a.T) and np.all(np.isfinite(a))
    return a


def score(a, v):
    """(residual ||A v - (v'Av) v||, Rayleigh quotient v'Av) in long double"""
    al, vl = a.astype(LD), np.asarray(v).astype(LD)
    av = al @ vl
    rq = vl @ av
    return float(np.sqrt(((av - rq * vl) ** 2).sum())), rq


def judge(a, v):
    """Check v against the criterion; returns (residual / U, deficit / U, limit_residual / U, limit_deficit / U, failures)."""
    d = a.shape[0]
    lam, vecs = np.linalg.eigh(a)
    lam_max, norm2 = lam[-1], float(np.abs(lam).max())
    U = EPS * np.sqrt(d) * norm2
    res, rq = score(a, v)
    res_ref, rq_ref = score(a, vecs[:, -1])
    dfc, dfc_ref = float(LD(lam_max) - rq), float(LD(lam_max) - rq_ref)
    lim_res, lim_dfc = 8 * max(U, res_ref), 8 * max(U, dfc_ref)
    fails = []
    nrm = float(np.sqrt((np.asarray(v).astype(LD) ** 2).sum()))
    if not np.all(np.isfinite(v)) or not abs(nrm - 1.0) <= 4 * EPS * np.sqrt(d):
        fails.append(f"| ||v|| - 1 | = {abs(nrm - 1.0):.3g}")
    big = np.abs(v).max()
    if not np.any(v[np.abs(v) >= big - 2 * np.spacing(big)] > 0):
        fails.append("the largest component is negative")
    if not res <= lim_res:
        fails.append(f"residual {res / U:.3g} U > limit {lim_res / U:.3g} U")
    if not dfc <= lim_dfc:
        fails.append(f"deficit {dfc / U:.3g} U > limit {lim_dfc / U:.3g} U")
    return res / U, dfc / U, lim_res / U, lim_dfc / U, fails
