"""The kernels of the packed exact sweep (option "exact_packed") through the hook cge_packed_gd_test: the extrema pass and the
generator of one alpha against the numpy reference of tests/packed_gd_ref.py, bit for bit -- every step up to the power is an
IEEE operation in dist()'s order, and the power of the reference is taken on the device by the element-wise hook."""
import numpy as np
import pytest

import packed_gd_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 256, 257, 321, 1000]  # one tile, ragged last tiles, odd N
DIMS = [1, 2, 16, 17, 33]                     # around the k-chunk (16) of the LDS staging
ALPHAS = [0.25, 3.0, 10.0]


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _check(ctx, emb, diag):
    """Every alpha and both powers on one input; D, its extrema and the normalisation are computed once."""
    n = emb.shape[0]
    D = ref.dist_matrix(emb, diag)
    lo, hi = ref.extrema_upper(D)
    x = ref.normalised(D, lo, hi)
    mask = ref.stored_mask(n)
    out = None
    for alpha in ALPHAS:
        for method in (1, 0):
            lo_hi, GD = ctx.packed_gd_test(emb, diag, alpha, method)
            exp = ctx.pow_test(x.ravel(), alpha, method).reshape(n, n)
            assert lo_hi[0] == lo and lo_hi[1] == hi, (lo_hi, lo, hi)
            assert np.array_equal(GD[mask], exp[mask], equal_nan=True), (n, emb.shape[1], alpha, method,
                                                                          int((GD[mask] != exp[mask]).sum()))
            assert np.all(np.isnan(GD[~mask]))  # the rest of each row is left as the caller filled it
            if n > 1:
                assert np.all(np.isfinite(GD[mask]))
            out = GD
    return (lo, hi), x, out


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_generator_and_extrema_zero_diagonal(ctx, n, d):
    """diag = zeros (exact mode on the original graph): lo = 0 comes from the diagonal."""
    rng = np.random.default_rng(1000 * n + d)
    emb = rng.standard_normal((n, d))
    (lo, hi), _, _ = _check(ctx, emb, np.zeros(n))
    assert lo == 0.0 and (n == 1 or hi > 0.0)


@pytest.mark.parametrize("d", [2, 17])
@pytest.mark.parametrize("n", [65, 257, 1000])
def test_generator_diagonal_below_every_pair(ctx, n, d):
    """diag = uniform(0.1, 0.2) with the points far apart: lo sits on the diagonal, hi off it."""
    rng = np.random.default_rng(7 * n + d)
    emb = rng.standard_normal((n, d)) + 10.0 * np.arange(n)[:, None]
    diag = rng.uniform(0.1, 0.2, n)
    (lo, hi), _, _ = _check(ctx, emb, diag)
    assert lo == diag.min() and hi > 0.2


@pytest.mark.parametrize("d", [2, 17])
@pytest.mark.parametrize("n", [65, 257, 1000])
def test_generator_largest_value_on_the_diagonal(ctx, n, d):
    """One diag entry beyond every pair distance: hi is on the diagonal and that entry's GD is exactly 0."""
    rng = np.random.default_rng(11 * n + d)
    emb = rng.standard_normal((n, d))
    diag = rng.uniform(0.1, 0.2, n)
    k = n - 2
    diag[k] = 1e3
    (lo, hi), x, GD = _check(ctx, emb, diag)
    assert hi == 1e3 and x[k, k] == 1.0 and GD[k, k] == 0.0


@pytest.mark.parametrize("d", [2, 17])
@pytest.mark.parametrize("n", [65, 257, 1000])
def test_generator_identical_rows(ctx, n, d):
    """Two identical rows in different tiles (where there are two): an off-diagonal 0 below the whole diagonal."""
    rng = np.random.default_rng(13 * n + d)
    emb = rng.standard_normal((n, d))
    a, b = 3, n - 1
    emb[b] = emb[a]
    diag = rng.uniform(0.1, 0.2, n)
    (lo, hi), x, GD = _check(ctx, emb, diag)
    assert lo == 0.0 and x[a, b] == 0.0 and GD[a, b] == 1.0
