"""References, a-priori error bounds and seeded inputs for the stage of a landmark run that turns an assignment v_to_l into the
landmark graph (src/landmarks.jl:387-463), as the hook cge_landmark_graph_test returns it (tests/test_gpu_landmark_graph.py;
tests/test_landmark_graph_ref.py checks this module itself on the CPU).  numpy only.

Aggregate.  The kernels add in ascending member order with unfused, rounded products, so the reference is plain SEQUENTIAL fp64
(np.cumsum behind a leading zero -- never np.sum, which adds pairwise) and the comparison is bit for bit:
    lw = sum w;  cen_c = (sum w x_c) / lw;  dist_i = sum_c (cen_c - x_ic)^2, columns in order;
    dii = sqrt(sum_i dist_i / lw) if lw > 0 else sum_i dist_i;  lcomm = the community of the last member.
A landmark whose weights are all zero has no centroid (0 / 0): NaN is compared for NaN.

Pair sums (landmark-pair matrix, vect_C, degrees).  The reference adds every bin in long double (np.add.at).  Unit and dyadic
weights add exactly in any order: np.array_equal.  General positive weights: the k terms of a bin are added in fp64 in an order
nobody fixes (LDS and memory atomics, trees over partial sums; additions of an exact zero commit no error).  Whatever the order,
every term passes through at most k - 1 rounded additions, each with relative error <= u = 2^-53 on a partial sum that is at
most the sum S of the (positive) terms times (1 + u)^(k - 2), so
    |fl(sum) - S| <= ((1 + u)^(k - 1) - 1) S <= (k - 1) u S / (1 - (k - 1) u)
(Higham, Accuracy and Stability, 4.2).  The long-double reference itself is within (k - 1) 2^-64 S of S, which is added.  A bin
of one term, and a bin nothing falls into, must be exact.  The degree sums of the directed score are row and column sums of the
RETURNED matrix over N entries in a tree order: the same bound with k = N.  star and the positive count are integers: exact.

Aggregate in another member order (the oracle comparison only).  With k members, abs_c = sum |w x_c| / lw:
    |cen'_c - cen_c| <= e_c = (2 k + 2) u abs_c         (k roundings on the numerator, k - 1 on lw, one division, slack 2)
    tot = sum_i dist_i moves by at most P = sum_i (2 sum_c |cen_c - x_ic| e_c + sum_c e_c^2) through the centroid, and by the
    relative F = (d + 2 k + 2) u (1.01) through its own d + 2 roundings per row and k - 1 per sum, lw's k - 1 and the division;
    dii' lies in [sqrt(max(tot - P, 0) (1 - F) / lw) (1 - 2 u), sqrt((tot + P) (1 + F) / lw) (1 + 2 u)].
No measured constant enters any bound."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
CLASSES = ("centred", "offset")
AGG_SIZES = (1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 513)  # around the 8- and 16-row unrolls and the 256-member staging chunk
AGG_WIDTHS = (1, 2, 15, 16, 17, 255, 256, 257, 512, 768, 1023, 1024, 1025, 1100)


# ---- aggregate --------------------------------------------------------------------------------------------------------------
def members_of(v2l0, N):
    """the members of every landmark (0-based ids), ascending"""
    order = np.argsort(v2l0, kind="stable")
    cuts = np.searchsorted(v2l0[order], np.arange(N + 1))
    return [order[cuts[l]:cuts[l + 1]] for l in range(N)]


def _seq_sum(terms, axis=0):
    """0 + t_0 + t_1 + ... in fp64, in order (the leading zero: -0.0 terms give the kernels' +0.0)"""
    terms = np.asarray(terms, dtype=np.float64)
    shape = list(terms.shape)
    shape[axis] = 1
    return np.take(np.cumsum(np.concatenate([np.zeros(shape), terms], axis=axis), axis=axis), -1, axis=axis)


def aggregate_ref(X, w, comm0, members):
    """(lemb (N, d), lweight (N,), dii (N,), lcomm (N,) int32) of the landmarks whose member lists (in the order to add in) are
    given: sequential fp64, rounded products"""
    N, d = len(members), X.shape[1]
    lemb, lw, dii, lcomm = np.empty((N, d)), np.empty(N), np.empty(N), np.empty(N, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for l, r in enumerate(members):
            x, wl = X[r], w[r]
            lw[l] = _seq_sum(wl)
            lemb[l] = _seq_sum(wl[:, None] * x) / lw[l]
            df = lemb[l] - x
            tot = _seq_sum(_seq_sum(df * df, axis=1))
            dii[l] = np.sqrt(tot / lw[l]) if lw[l] > 0 else tot
            lcomm[l] = comm0[r[-1]]
    return lemb, lw, dii, lcomm


def same_bits(a, b):
    """equal bit for bit, except that NaN matches NaN (and +0.0 is not -0.0)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan))


def reorder_ratios(X, w, members, lemb, dii):
    """Worst (error / bound) of centroids and d_ii computed in fp64 in ANY member order, against long double: (cen, dii).
    Landmarks of positive weight only."""
    worst_c = worst_d = 0.0
    d = X.shape[1]
    for l, r in enumerate(members):
        k = len(r)
        x, wl = X[r].astype(LD), w[r].astype(LD)
        lw = wl.sum()
        cen = (wl[:, None] * x).sum(0) / lw
        e = (2 * k + 2) * U * np.abs(wl[:, None] * x).sum(0) / lw
        worst_c = max(worst_c, _ratio(lemb[l] - cen, e))
        df = cen - x
        tot = (df * df).sum()
        P = (2 * np.abs(df) @ e).sum() + k * (e * e).sum()
        F = (d + 2 * k + 2) * U * 1.01
        hi = np.sqrt((tot + P) * (1 + F) / lw) * (1 + 2 * U)
        lo = np.sqrt(max(tot - P, LD(0)) * (1 - F) / lw) * (1 - 2 * U)
        mid = np.sqrt(tot / lw)
        got = LD(dii[l])
        worst_d = max(worst_d, _ratio(got - mid, hi - mid if got >= mid else mid - lo))
    return worst_c, worst_d


def _ratio(err, bound):
    """max over the elements of |err| / bound; an error where the bound is 0 counts as infinite"""
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    bad = (bound == 0) & (err != 0)
    if bad.any() or not np.all(np.isfinite(err)):
        return float("inf")
    return float((err / np.where(bound == 0, 1, bound)).max())


def make_aggregate_problem(cls, d, seed=0):
    """(X (n, d), w (n,), comm0 (n,), v2l (n,) 1-based, N) -- landmarks of AGG_SIZES members, interleaved over the rows, then one
    landmark spanning two communities (its last member in the second) and one of zero total weight; weights over many magnitudes
    with zeros inside the landmarks.  Every landmark has a positive weight except the last."""
    rng = np.random.default_rng([seed, d, CLASSES.index(cls)])
    sizes = list(AGG_SIZES) + [40, 5]
    N, n = len(sizes), sum(sizes)
    v2l = rng.permutation(np.repeat(np.arange(1, N + 1), sizes))
    X = rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, d)
    if cls == "offset":  # mean >> spread
        X = 1e3 + 1e-3 * rng.standard_normal((n, d))
    w = np.exp(rng.uniform(-12.0, 12.0, n))
    w[rng.random(n) < 0.15] = 0.0
    comm0 = (v2l - 1) % 7
    mem = members_of(v2l - 1, N)
    for l in range(N - 1):
        if w[mem[l]].sum() == 0:
            w[mem[l][0]] = 1.5
    w[mem[N - 1]] = 0.0
    two = mem[N - 2]
    comm0[two[: len(two) // 2]] = 8
    comm0[two[len(two) // 2:]] = 9
    return np.ascontiguousarray(X), w, comm0.astype(np.int64), v2l.astype(np.int64), N


# ---- pair sums --------------------------------------------------------------------------------------------------------------
def pair_index(a, b, K, directed, packed=False):
    """flat bin of the 0-based pair (a, b) among K ids: K x K row-major (undirected: (min, max), the upper triangle), or with
    packed (vect_C, undirected) the packed upper triangle of src/auxilary.jl:57-59"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if not directed:
        a, b = np.minimum(a, b), np.maximum(a, b)
    if packed and not directed:
        return K * a - a * (a - 1) // 2 + (b - a)
    return a * K + b


def bin_sums(flat, w, length=None):
    """(bins (unique flat indices), S (their long-double sums, np.add.at), k (their term counts))"""
    bins, inv = np.unique(flat, return_inverse=True)
    S = np.zeros(len(bins), dtype=LD)
    np.add.at(S, inv, np.asarray(w).astype(LD))
    return bins, S, np.bincount(inv, minlength=len(bins))


def dense(bins, S, length):
    out = np.zeros(length)
    out[bins] = S.astype(np.float64)
    return out


def sum_bound(S, k):
    """|fl(sum) - S| for k positive terms added in fp64 in any order, plus the long-double reference's own error"""
    k1 = np.maximum(np.asarray(k, dtype=LD) - 1, 0)
    return k1 * U * S / (1 - k1 * U) + k1 * LD(2.0) ** -64 * S


def bins_ratio(got_flat, bins, S, k):
    """worst |got - S| / bound over the bins; inf when an entry outside the bins is not zero or a one-term bin is not exact"""
    got_flat = np.asarray(got_flat).ravel()
    at = got_flat[bins]
    if np.count_nonzero(got_flat) != np.count_nonzero(at):  # (something outside the bins)
        return float("inf")
    return _ratio(at.astype(LD) - S, sum_bound(S, k))


def degrees_ref(W):
    """from the matrix itself: (deg_out, deg_in) in long double, star (row + column counts of positive entries)"""
    WL = W.astype(LD)
    pos = W > 0
    return WL.sum(1), WL.sum(0), (pos.sum(1) + pos.sum(0)).astype(np.int32)


def degrees_ratio(got, ref):
    N = len(ref)
    return _ratio(np.asarray(got).astype(LD) - ref, sum_bound(ref, np.full(N, N)))


def positive_ref(W, directed):
    return int(np.count_nonzero((W if directed else np.triu(W)) > 0))


def edge_weights(kind, m, rng):
    """unit: ones; dyadic: k / 4 (exact sums in any order); general: positive fp64 over three magnitudes"""
    if kind == "unit":
        return np.ones(m)
    if kind == "dyadic":
        return rng.integers(1, 9, m) / 4.0
    return np.exp(rng.uniform(-3.0, 3.0, m))


# ---- the graphs of the GPU tests ----------------------------------------------------------------------------------------------
UBLOCK, VBLOCK, CHUNK = 131072, 32768, 16384  # the blocked edge list: source block, target block, longest chunk


def tile_census(src0, dst0, n):
    """{(source block, target block): edges} of the tiles that hold an edge, and the number of chunks the blocked edge list cuts
    them into (a tile of len edges: ceil(len / 16384) equal pieces)"""
    nbv = (n + VBLOCK - 1) // VBLOCK
    t, cnt = np.unique((src0 // UBLOCK) * nbv + dst0 // VBLOCK, return_counts=True)
    tiles = {(int(x) // nbv, int(x) % nbv): int(c) for x, c in zip(t, cnt)}
    return tiles, int(sum((c + CHUNK - 1) // CHUNK for c in tiles.values()))


def make_graph(name, seed=0):
    """(n, src0, dst0): 0-based edges of one of the three graphs.
    small:  n = 3000, m = 20 000 in one tile (two chunks); self-loops, repeated edges, both orientations of a pair.
    bounds: n = 140 000 = 2 source blocks x 5 target blocks, three tiles with edges -- (0, 1) with exactly 16384 (one chunk; its
            sources lie outside its target block, so that an assignment can file all of it under ONE landmark pair), (1, 2) with
            16385 (two pieces) and (0, 4) with a single edge; vertices 0, 32767, 65536, 131071, 131072 and n - 1 are sources,
            32768, 65535, 65536 and n - 1 targets.
    chunks: n = 2 200 000 = 17 x 68 = 1156 tiles with 4 or 5 edges each: more than 1024 chunks."""
    rng = np.random.default_rng([seed, ("small", "bounds", "chunks").index(name)])
    if name == "small":
        n = 3000
        src, dst = rng.integers(0, n, 18800), rng.integers(0, n, 18800)
        src[:200] = dst[:200]
        src = np.concatenate([src, src[200:600], dst[600:1400]])
        dst = np.concatenate([dst, dst[200:600], src[600:1400]])
        return n, src, dst
    if name == "bounds":
        n = 140_000
        sa = np.concatenate([[0, 32767, 65536, 131071], rng.integers(0, VBLOCK, 8000), rng.integers(2 * VBLOCK, UBLOCK, 8380)])
        da = np.concatenate([[VBLOCK, 2 * VBLOCK - 1], rng.integers(VBLOCK, 2 * VBLOCK, 16382)])
        sb = np.concatenate([[UBLOCK, n - 1], rng.integers(UBLOCK, n, 16383)])
        db = np.concatenate([[2 * VBLOCK], rng.integers(2 * VBLOCK, 3 * VBLOCK, 16384)])
        src, dst = np.concatenate([sa, sb, [131071]]), np.concatenate([da, db, [n - 1]])
        p = rng.permutation(len(src))
        return n, src[p], dst[p]
    n = 2_200_000
    nbu, nbv = (n + UBLOCK - 1) // UBLOCK, (n + VBLOCK - 1) // VBLOCK
    src, dst = [], []
    for bu in range(nbu):
        for bv in range(nbv):
            k = 4 + (bu * nbv + bv) % 3 // 2
            src.append(rng.integers(bu * UBLOCK, min(n, (bu + 1) * UBLOCK), k))
            dst.append(rng.integers(bv * VBLOCK, min(n, (bv + 1) * VBLOCK), k))
    src, dst = np.concatenate(src), np.concatenate(dst)
    p = rng.permutation(len(src))
    return n, src[p], dst[p]


def assignments(name, n, N, rng):
    """[(label, v2l (n,) 1-based)]: random; contiguous (id // k: a whole chunk lands in a few tile rows, runs far beyond 64 keys);
    sparse (random over every third id: landmarks without a member); on `bounds` also pair: the target block of the 16384-edge
    tile in landmark N, everything else in landmark 1 -- 16384 additions into one cell"""
    out = [("random", rng.integers(1, N + 1, n))]
    if N >= 2:
        out.append(("contiguous", np.arange(n) // ((n + N - 1) // N) + 1))
        out.append(("sparse", np.full(n, N) if N < 6 else 3 * rng.integers(0, N // 3, n) + 2))
        if name == "bounds":
            v = np.ones(n, dtype=np.int64)
            v[VBLOCK:2 * VBLOCK] = N
            out.append(("pair", v))
    return [(a, np.ascontiguousarray(v, dtype=np.int64)) for a, v in out]
