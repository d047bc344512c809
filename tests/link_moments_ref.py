"""Reference, a-priori bound and named inputs of cge_link_moments (no GPU, numpy only).

The reference evaluates the definitions of include/cge_hip.h over EVERY pair in numpy.longdouble:

    p(i, j) = f_out[i] f_in[j] max(0, 1 - dist(i, j) / hi)^alpha,      q = min(p, 1)
    deg_out[i] = sum_{j != i} p(i, j),   deg_in[j] = sum_{i != j} p(i, j),   B[bin] = sum p,   V[bin] = sum q (1 - q)

dist is src/auxilary.jl:14-20 in its own arithmetic -- a Float64 sum over the coordinates in ascending order, a Float64 root --
and the base b = fl(1 - fl(dist / hi)) is taken in Float64 as well: these three are the model's definition of the base
(cge_link_prob's link_p takes them so, and a power with alpha < 1 is not Lipschitz at b = 0, so "the" base has to be one fixed
number).  The power, the products and every sum are long double.

The bound of an output that sums the pair set S is

    bound = c_pair * sum_S f_out[i] f_in[j]  +  |S| 2^-53 * sum_S p_ref

with c_pair derived below from the kernel's DOCUMENTED arithmetic (kernels_link.hip, "cge_link_moments"), not from anything the
GPU returned; the second term is a deliberately loose cover for the fixed-order fp64 summation.  The bound is absolute per pair
(relative to f f, not to the bin's own sum): a bin of far-apart communities has a tiny B and the same tolerance."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
THETA = 2.0 ** -10  # the kernel's thresholds: g >= THETA (r_i + r_j) and base >= BETA take the Gram value
BETA = 2.0 ** -10
C_PAIR_CAP = 1e-8


def c_pair(d, alpha):
    """Per pair |p_kernel - p_ref| <= c_pair f_out[i] f_in[j].

    Fast pairs: the Gram value g is within e (r_i + r_j), e = (dpad + 16) 2^-52, dpad = d rounded up to 16, of the squared
    distance of the fp64 rows; the reference's fp64 dist^2 is within (d + 6) 2^-53 of it relatively and dist^2 <= 2 (r_i + r_j),
    so g is within e' (r_i + r_j), e' = e + (d + 6) 2^-52, of the REFERENCE's squared distance.  With g >= THETA (r_i + r_j) that
    is e' / THETA relatively, e' / (2 THETA) for the root, and -- x = dist / hi <= 1 + 1e-12 on this branch -- the same absolutely
    for the base, plus three roundings (root, quotient, difference).  Both bases are above BETA / 2, where the derivative of
    b^alpha is at most alpha (alpha >= 1) or alpha (BETA / 2)^(alpha - 1) (alpha < 1).  The power itself is within two ulp, the
    two products one each, the clamp to q and q (1 - q) are 1-Lipschitz: six ulp for all of that.
    Exact pairs (link_p from the rows) share the reference's base bit for bit: the six ulp alone."""
    dpad = (int(d) + 15) // 16 * 16
    e = (dpad + 16) * 2.0 ** -52 + (int(d) + 6) * 2.0 ** -52
    base_err = e / (2.0 * THETA) * (1.0 + 1e-9) + 3 * U
    deriv = float(alpha) if alpha >= 1.0 else float(alpha) * (BETA / 2.0) ** (float(alpha) - 1.0)
    return deriv * base_err + 6 * U


def dist64(X):
    """(n, n) Float64: dist() of every pair, the sum in ascending coordinate order, 0 on the diagonal."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    s = np.zeros((n, n))
    for k in range(d):
        df = X[:, None, k] - X[None, :, k]
        s = s + df * df
    D = np.sqrt(s)
    np.fill_diagonal(D, 0.0)
    return D


def table(c):
    """(P, FF): p of every ordered pair (diagonal included: p(i, i) = f_out[i] f_in[i]) and f_out[i] f_in[j], long double."""
    D = dist64(c["X"])
    b = 1.0 - D / float(c["hi"])  # Float64, as the definition takes it
    b = np.where(b < 0.0, 0.0, b)
    FF = np.asarray(c["fo"], LD)[:, None] * np.asarray(c["fi"], LD)[None, :]
    return FF * np.power(b.astype(LD), LD(c["alpha"])), FF


def bin_index(comm, C, directed):
    """(n, n) int64: the 0-based bin of every ordered pair in the sweep's layout (comm 1-based)."""
    a, b = np.asarray(comm, np.int64)[:, None], np.asarray(comm, np.int64)[None, :]
    if directed:
        return (a - 1) * C + (b - 1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return C * (lo - 1) - (lo - 1) * (lo - 2) // 2 + hi - lo


def pair_mask(n, directed, diag):
    """The pair set of the bins: i < j (directed: i != j), with the diagonal under diag."""
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    m = (i != j) if directed else (i < j)
    return m | (i == j) if diag else m


def _binsum(idx, w, L):
    out = np.zeros(L, LD)
    np.add.at(out, idx, w)
    return out


def moments(c, diag=False):
    """The reference and its bound: {"deg_out", "deg_in", "B", "V"} (long double) and under "bound" the same keys (float64), plus
    "saturated" (pairs of the bins' set with p > 1), "pairs" (the set's size without the diagonal), "L"."""
    P, FF = table(c)
    n, C, directed = len(P), int(c["C"]), bool(c["directed"])
    L = C * C if directed else C * (C + 1) // 2
    cp = c_pair(np.asarray(c["X"]).shape[1], c["alpha"])
    S = pair_mask(n, directed, diag)
    off = ~np.eye(n, dtype=bool)
    Dg = np.eye(n, dtype=bool) if diag else np.zeros((n, n), bool)
    Q = np.minimum(P, LD(1))
    Vt = Q * (LD(1) - Q)
    if directed:
        Mo = off | Dg
        deg_out, deg_in = (P * Mo).sum(1), (P * Mo).sum(0)
        ffo, ffi = (FF * Mo).sum(1), (FF * Mo).sum(0)
        cnt = Mo.sum(1)
    else:  # p is symmetric: the row of the full table, the diagonal once
        Mo = off | Dg
        deg_out = deg_in = (P * Mo).sum(1)
        ffo = ffi = (FF * Mo).sum(1)
        cnt = Mo.sum(1)
    idx = bin_index(c["comm"], C, directed)
    B, V = _binsum(idx[S], P[S], L), _binsum(idx[S], Vt[S], L)
    ffb, nb = _binsum(idx[S], FF[S], L), _binsum(idx[S], np.ones(int(S.sum()), LD), L)
    bound = {"deg_out": (cp * ffo + cnt * U * deg_out).astype(np.float64),
             "deg_in": (cp * ffi + cnt * U * deg_in).astype(np.float64),
             "B": (cp * ffb + nb * U * B).astype(np.float64), "V": (cp * ffb + nb * U * B).astype(np.float64)}
    return {"deg_out": deg_out, "deg_in": deg_in, "B": B, "V": V, "bound": bound, "saturated": int((P[S] > 1).sum()),
            "pairs": n * (n - 1) if directed else n * (n - 1) // 2, "L": L, "c_pair": cp, "P": P}


def moments_loops(c, diag=False):
    """The same definitions as plain Python double loops (tiny inputs only): (deg_out, deg_in, B, V) as float lists."""
    X, fo, fi = np.asarray(c["X"], np.float64), c["fo"], c["fi"]
    n, C, directed, hi, alpha = len(X), int(c["C"]), bool(c["directed"]), float(c["hi"]), float(c["alpha"])
    L = C * C if directed else C * (C + 1) // 2
    do, di, B, V = [0.0] * n, [0.0] * n, [0.0] * L, [0.0] * L

    def p(i, j):
        dist = 0.0 if i == j else float(np.sqrt(sum((X[i, k] - X[j, k]) ** 2 for k in range(X.shape[1]))))
        return float(fo[i]) * float(fi[j]) * max(0.0, 1.0 - dist / hi) ** alpha

    for i in range(n):
        for j in range(n):
            if i == j and not diag:
                continue
            v = p(i, j)
            do[i] += v
            di[j] += v
            if directed or i <= j:
                a, b = int(c["comm"][i]), int(c["comm"][j])
                if not directed and a > b:
                    a, b = b, a
                at = (a - 1) * C + (b - 1) if directed else C * (a - 1) - (a - 1) * (a - 2) // 2 + b - a
                q = min(v, 1.0)
                B[at] += v
                V[at] += q * (1.0 - q)
    if not directed:
        di = do
    return do, di, B, V


def vect_C(c):
    """The sweep's vect_C of the case's edges (integer weights: exact in any order) by numpy.bincount."""
    C, directed = int(c["C"]), bool(c["directed"])
    L = C * C if directed else C * (C + 1) // 2
    e = np.asarray(c["edges"], np.int64)
    idx = bin_index(c["comm"], C, directed)[e[:, 0], e[:, 1]]
    return np.bincount(idx, weights=np.asarray(c["weights"], np.float64), minlength=L)


# ---- the named inputs ---------------------------------------------------------------------------------------------------------------
def _case(n, d, directed, alpha, comm, seed, scale=0.6, hi_factor=1.0, X=None, C=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) if X is None else X
    fo = scale * (0.1 + 0.9 * rng.random(n))
    fi = scale * (0.1 + 0.9 * rng.random(n)) if directed else fo
    m = 3 * n
    edges = rng.integers(0, n, size=(m, 2))
    comm = np.asarray(comm, np.int64)
    return dict(X=X, fo=fo, fi=fi, alpha=float(alpha), hi=float(dist64(X).max() * hi_factor), directed=bool(directed), comm=comm,
                C=int(comm.max() if C is None else C), edges=edges, weights=rng.integers(1, 4, size=m).astype(np.float64))


def _sizes(*sizes):
    return np.repeat(np.arange(1, len(sizes) + 1), sizes)


def _shuffled(n, C, seed):
    rng = np.random.default_rng(seed)
    comm = np.arange(n) % C + 1
    rng.shuffle(comm)
    return comm


def _near_rows(n, d, seed):
    """Repeated rows and rows 1e-9 apart: pairs the Gram value says nothing about."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X[10:20] = X[0]
    X[20:30] = X[1] + 1e-9 * rng.standard_normal((10, d))
    return X


def cases():
    """name -> case.  Shapes: the smallest at which each path can go wrong -- one partial tile (5), two tiles with one nearly
    empty (129), several work items (300: three, one a partial block; 700: six), d of 3, 64 and 130 (dpad 16, 64, 144), both
    layouts, alpha 0.25 / 3 / 10."""
    c = {}
    c["n5_one_tile"] = _case(5, 3, False, 3.0, _sizes(5), 1)
    c["n129_two_tiles_dir"] = _case(129, 64, True, 0.25, _sizes(129), 2)
    c["n300_boundary_in_tile"] = _case(300, 3, False, 10.0, _sizes(1, 170, 129), 3)
    c["n300_boundary_in_tile_dir"] = _case(300, 130, True, 0.25, _sizes(1, 170, 129), 4)
    c["n700_shuffled_c7"] = _case(700, 64, False, 3.0, _shuffled(700, 7, 5), 5)
    c["n700_shuffled_c7_dir"] = _case(700, 3, True, 10.0, _shuffled(700, 7, 6), 6)
    c["n700_pairs_of_vertices"] = _case(700, 3, False, 3.0, np.arange(700) // 2 + 1, 7)
    c["n300_pairs_of_vertices_dir"] = _case(300, 64, True, 3.0, _shuffled(300, 150, 8), 8)
    c["n129_empty_community"] = _case(129, 130, False, 0.25, np.array([1, 3, 4])[np.arange(129) % 3], 9)
    c["n300_near_rows"] = _case(300, 64, False, 0.25, _sizes(100, 200), 10, X=_near_rows(300, 64, 10))
    c["n300_near_rows_dir"] = _case(300, 3, True, 10.0, _sizes(100, 200), 11, X=_near_rows(300, 3, 11))
    c["n300_small_hi_dir"] = _case(300, 3, True, 3.0, _sizes(150, 150), 12, hi_factor=0.6)
    c["n129_small_hi"] = _case(129, 64, False, 0.25, _sizes(64, 65), 13, hi_factor=0.9)
    z = _case(129, 3, True, 3.0, _sizes(60, 69), 14)
    z["fo"][[0, 5, 128]] = 0.0
    z["fi"][[1, 5, 127]] = 0.0
    c["n129_zero_factors_dir"] = z
    c["n300_saturated"] = _case(300, 3, False, 3.0, _sizes(1, 170, 129), 15, scale=6.0)
    c["n300_saturated_dir"] = _case(300, 64, True, 0.25, _sizes(100, 200), 16, scale=3.0)
    c["n700_draw"] = _case(700, 3, False, 3.0, _sizes(200, 250, 250), 17, scale=0.5)
    return c
