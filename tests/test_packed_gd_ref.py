"""The numpy reference of the packed exact sweep's kernel tests (tests/packed_gd_ref.py) against the oracle's dist()."""
import ctypes as C

import numpy as np

import packed_gd_ref as ref


def test_helper_distances_are_the_oracles_bits(test115):
    """On the 115-vertex fixture's embedding the helper's D equals the oracle's dist() on every pair, bit for bit."""
    from oracle import oracle as orc

    emb = np.asarray(test115["embedding"], dtype=np.float64)
    n, d = emb.shape
    L = orc.lib()
    L.orc_dist.restype = C.c_double
    L.orc_dist.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]
    _, flat = orc._f(emb)
    exp = np.array([[L.orc_dist(i + 1, j + 1, orc._ptr(flat), n, d) for j in range(n)] for i in range(n)])
    D = ref.dist_matrix(emb, np.zeros(n))
    assert np.array_equal(D.view(np.uint64), exp.view(np.uint64))
    diag = np.linspace(0.1, 0.2, n)
    D2 = ref.dist_matrix(emb, diag)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(D2[off], exp[off]) and np.array_equal(np.diag(D2), diag)


def test_helper_extrema_normalisation_and_mask():
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((70, 3))
    diag = np.full(70, 50.0)
    diag[5] = 60.0
    D = ref.dist_matrix(emb, diag)
    lo, hi = ref.extrema_upper(D)
    assert hi == 60.0 and lo == D[np.triu_indices(70, 1)].min()
    x = ref.normalised(D, lo, hi)
    assert x[5, 5] == 1.0 and x.min() == 0.0
    m = ref.stored_mask(70)
    assert m[0, 69] and not m[69, 0] and m[63, 0] and m[69, 64] and not m[64, 63] and m.sum() == 70 * 71 // 2 + 64 * 63 // 2 + 6 * 5 // 2
