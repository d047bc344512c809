"""The packed form of an exact sweep (option "exact_packed") in numpy: D by dist()'s own arithmetic, its extrema over j >= i, the
normalisation -- every step an IEEE operation that numpy and the device round alike, so the kernels are compared bit for bit.
The power itself is taken on the device by the existing element-wise hook (`Context.pow_test`)."""
import numpy as np


def dist_matrix(emb, diag):
    """D[i, j] = dist(i, j, embed) (src/auxilary.jl:14-20): acc = acc + (a - b) * (a - b) in ascending k, then sqrt (numpy
    has no FMA, so these are dist()'s bits); `diag` on the diagonal (src/divergence.jl:79-91)."""
    emb = np.ascontiguousarray(emb, dtype=np.float64)
    n, d = emb.shape
    acc = np.zeros((n, n))
    for k in range(d):
        col = emb[:, k]
        df = col[:, None] - col[None, :]
        acc = acc + df * df
    D = np.sqrt(acc)
    D[np.arange(n), np.arange(n)] = np.asarray(diag, dtype=np.float64)
    return D


def extrema_upper(D):
    """lo, hi = extrema(D) over j >= i (src/divergence.jl:92)."""
    up = D[np.triu_indices(D.shape[0])]
    return up.min(), up.max()


def normalised(D, lo, hi):
    """(D - lo) / (hi - lo) (src/divergence.jl:93): two operations per element."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (D - lo) / (hi - lo)


def stored_mask(n):
    """The elements the packed form stores: j >= i, and both halves of the diagonal 64 x 64 tiles."""
    i = np.arange(n)
    return (i[None, :] >= i[:, None]) | ((i[None, :] // 64) == (i[:, None] // 64))


def reference(ctx, emb, diag, alpha, pow_method):
    """((lo, hi), GD) as the packed form must produce them; GD is the full matrix (compare under stored_mask)."""
    D = dist_matrix(emb, diag)
    lo, hi = extrema_upper(D)
    x = normalised(D, lo, hi)
    return np.array([lo, hi]), ctx.pow_test(x.ravel(), alpha, pow_method).reshape(D.shape)
