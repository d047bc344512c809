"""The point-set diameter `hi` (src/divergence.jl:104-113) where kernels go wrong: near-tied, extreme-range and
odd-shaped inputs (run with -m gpu on an MI355X).

Every expected value is computed here: `orc.max_pair_dist` (sequential sums, the reference's own arithmetic) gives the
bits of `hi`; `np.longdouble` gives the true squared distances the bound matrix must dominate.

B1  the bound matrix of the pruned diameter, pass by pass, against the long double maximum (cge_diameter_bounds_test);
B2  the fitness verdict of the low-precision bound passes, through the hook and through `score`;
B3  near-ties: inputs where many pairs lie within a few ulp of the maximum, so that ranking pairs by the Gram formula
    r_i + r_j - 2 <x_i, x_j> and taking the value of the winner by sequential sums need not give the largest sequential sum;
B4  the shapes test_max_pair_dist_kernel (test_gpu_parity.py) leaves out.
"""
import numpy as np
import pytest

from diameter_ref import dist_seq

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


def _load(ctx, emb):
    ctx.set_graph(np.array([[1, 2]]), [1.0], emb.shape[0])
    ctx.set_embedding(emb)


# ---------------------------------------------------------------------------------------------------------------
# B1. bound matrix
D_ALL = [1, 2, 15, 16, 17, 31, 33, 64, 65, 96, 97, 127, 128]
D_WIDE = [129, 200, 256, 333, 512]
NS = [2, 17, 128, 129, 1000, 5000]
PROFILES = ["singletons", "mixed", "one_big", "sixteens"]
KINDS = ["normal", "offset", "scales", "zero_column", "duplicates"]


def _sizes(profile, n):
    if profile == "singletons" or n <= 3:
        return [1] * n
    if profile == "one_big":
        return [n - 3, 1, 1, 1]
    if profile == "sixteens":
        return [16] * (n // 16) + ([n % 16] if n % 16 else [])
    out, left, k = [], n, 0  # "mixed": 1, 1, 1, 15, 16, 17 (six landmarks in the first 128-row tile), 113, ... repeated
    pat = [1, 1, 1, 15, 16, 17, 113]
    while left > 0:
        s = min(left, pat[k % len(pat)])
        out.append(s)
        left -= s
        k += 1
    return out


def _data(kind, rng, n, d):
    X = rng.standard_normal((n, d))
    if kind == "offset":
        X += 1e4
    elif kind == "scales":
        X *= 2.0 ** np.linspace(-30, 30, d) if d > 1 else 2.0 ** 30
    elif kind == "zero_column":
        X[:, d // 2] = 0.0
    elif kind == "duplicates":
        X = np.repeat(X[: (n + 4) // 5], 5, axis=0)[:n]
    return np.asfortranarray(X)


def _pexact(xc, mc, v2l, N):
    """Pexact[a][r] = max over the members i of a of |x_i - m_r|^2, rmax[a] = max |x_i|^2, in long double."""
    xl, ml = xc.astype(LD), mc.astype(LD)
    P = np.zeros((N, ml.shape[0]), dtype=LD)
    D = np.empty((xl.shape[0], ml.shape[0]), dtype=LD)
    for r in range(ml.shape[0]):
        t = xl - ml[r]
        D[:, r] = (t * t).sum(1)
    np.maximum.at(P, v2l - 1, D)
    rmax = np.zeros(N, dtype=LD)
    np.maximum.at(rmax, v2l - 1, (xl * xl).sum(1))
    return P, rmax, (ml * ml).sum(1)


def _pass_e(pass_, dpad):
    """The passes' own margins e as their launch wrappers compute them (kernels_dist.hip (2), (2b), (2c))."""
    if pass_ == 2:
        return 1.05 * (3.0 * ((dpad + 31) // 32 * 32 + 2) * 2.0 ** -23 + 3.2 * 2.0 ** -16)
    if pass_ == 1:
        return 1.01 * (dpad + 3) * 2.0 ** -24
    return (dpad + 8) * 2.0 ** -52


def _expected_pass(xc, mc, pass_):
    """The fitness verdict (diameter_host.cpp): a low-precision pass runs when every centred value is 0 or in [2^-100, 2^100)
    and some value reaches 2^-40; otherwise the fp64 pass."""
    a = np.abs(np.concatenate([xc.ravel(), mc.ravel()]))
    bad = (~(a < 2.0 ** 100) | ((a != 0) & (a < 2.0 ** -100))).any()
    return pass_ if (not bad and (a >= 2.0 ** -40).any()) else 0


def _check_bounds(ctx, emb, v2l, N, lcomm, C, pass_, cache, what, upper=True):
    P, ran, ref, mean = ctx.diameter_bounds_test(v2l, N, lcomm, C, pass_)
    assert P.shape == (N, C if C >= 32 else N), what
    key = C if C >= 32 else 0  # the reference points: C community centroids, or the landmarks' own
    xc, mc = emb - mean, ref - mean  # the device centres with the same single subtraction
    assert ran == _expected_pass(xc, mc, pass_), (what, ran)
    if key not in cache:
        cache[key] = _pexact(xc, mc, v2l, N)
    Pex, rmax, mn = cache[key]
    Pl = P.astype(LD)
    low = Pl < Pex * (1 - LD(2.0) ** -53)  # no slack beyond rounding Pexact to a double
    assert not low.any(), (what, int(low.sum()), float((Pex - Pl)[low].max()), np.argwhere(low)[:3].tolist())
    if upper:
        scale = rmax[:, None] + mn[None, :]
        dpad = (emb.shape[1] + 15) // 16 * 16
        tol = (2 * _pass_e(ran, dpad) + (dpad + 8) * 2.0 ** -52) * scale
        high = Pl > Pex + tol
        assert not high.any(), (what, int(high.sum()), float(((Pl - Pex) / np.maximum(scale, LD(1e-300)))[high].max()))
    return P, ran


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("d", D_ALL + D_WIDE)
def test_bound_matrix_dominates_long_double_maximum(ctx, d, profile):
    """Every pass that applies returns P >= Pexact entry by entry (no excluded entry) and no looser than its documented
    margin: P <= Pexact + 2 e (|x|^2_max,a + |m_r|^2) plus the fp64 rounding of the norms.  The bf16 pass is refused for
    d > 128.  Over the six n the data kind cycles (two kinds per n up to 129, one above), so that each (d, profile) sees every kind
    and both sorts of reference points (landmarks for C < 32, communities for C >= 32); the landmark reference points are
    used where N <= 200, because Pexact costs n N d long double operations."""
    from cge.jl_amd import api

    di, pi = (D_ALL + D_WIDE).index(d), PROFILES.index(profile)
    for ni, n in enumerate(NS):
        rng = np.random.default_rng(1000 * d + 10 * pi + ni)
        sizes = _sizes(profile, n)
        N = len(sizes)
        v2l = np.empty(n, dtype=np.int64)
        v2l[rng.permutation(n)] = np.repeat(np.arange(1, N + 1), sizes)
        kinds = [KINDS[(di + pi + ni) % 5], KINDS[(di + pi + ni + 2) % 5]] if n <= 129 else [KINDS[(di + pi + ni) % 5]]
        cs = [c for c in (1, 31, 32, 150) if c <= N and (c >= 32 or N <= 200)]
        if n == 5000 and d > 128 and 32 in cs:
            cs = [32]
        for kind in kinds:
            emb = _data(kind, rng, n, d)
            _load(ctx, emb)
            cache = {}
            for C in cs:
                lcomm = np.arange(N) % C + 1
                for pass_ in (0, 1, 2):
                    what = (d, profile, n, kind, C, pass_)
                    if pass_ == 2 and d > 128:
                        with pytest.raises(api.CGEError) as ei:
                            ctx.diameter_bounds_test(v2l, N, lcomm, C, 2)
                        assert ei.value.code == -7, what  # CGE_E_ARG (include/cge_hip.h)
                        continue
                    _check_bounds(ctx, emb, v2l, N, lcomm, C, pass_, cache, what)


# ---------------------------------------------------------------------------------------------------------------
# B2. fitness verdict
def _verdict_cases():
    from cge.jl_amd import synth

    g = synth.abcd_like(3000, 30000, 10, 32, seed=7)
    base = np.array(g["embedding"])
    out = {}
    x = base.copy(); x[17, 3] = 2.0 ** 101
    out["one_2p101"] = (x, False)
    x = base.copy(); x[:, 5] = 0.0; x[99, 5] = 2.0 ** -101
    out["one_2m101"] = (x, False)
    out["all_2m50"] = (base * 2.0 ** -50, False)
    x = base.copy(); x[17, 3] = 2.0 ** 99
    out["one_2p99"] = (x, True)
    out["all_2p70"] = (base * 2.0 ** 70, True)
    return g, out


@pytest.mark.parametrize("case", ["one_2p101", "one_2m101", "all_2m50", "one_2p99", "all_2p70"])
def test_fitness_verdict_and_hi_on_extreme_ranges(ctx, orc, case):
    """A centred value beyond 2^+-100, or none reaching 2^-40: the fp64 pass runs instead of the requested one.  Inside the
    range the requested pass runs even where its f32 accumulators overflow (entries of 1e300 / Inf are upper bounds).  In
    every case the bounds dominate Pexact and `hi` has the oracle's bits: brute force, pruned only, automatic, with each
    setting of diameter_f32."""
    g, cases = _verdict_cases()
    x, fit = cases[case]
    emb = np.asfortranarray(x)
    n = emb.shape[0]
    exp = orc.max_pair_dist(emb)
    assert np.isfinite(exp) and exp > 0
    _load(ctx, emb)
    rng = np.random.default_rng(3)
    N = 60
    v2l = rng.permutation(np.repeat(np.arange(1, N + 1), n // N))
    for C in (4, 40):
        cache = {}
        for pass_ in (0, 1, 2):
            # (the upper side is B1's subject; with overflowed accumulators there is none to check)
            _, ran = _check_bounds(ctx, emb, v2l, N, np.arange(N) % C + 1, C, pass_, cache, (case, C, pass_), upper=False)
            assert ran == (pass_ if fit else 0), (case, C, pass_, ran)
    hi, ai, aj = ctx.max_pair_dist()
    assert hi == exp and dist_seq(emb[ai - 1], emb[aj - 1])[0] == exp, (case, hi, exp)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], emb)
    try:
        for f32 in (0, 1, 2):
            ctx.set_option("diameter_f32", f32)
            for opt in (1, 2, 0):
                ctx.set_option("diameter", opt)
                ctx.score(g["clusters"], 60, 4, "rss", seed=3, auc_samples=2000)
                got, path, pairs, tiles = ctx.last_diameter()
                assert got == exp, (case, f32, opt, got, exp, path, pairs, tiles)
                if opt == 2:
                    assert path == "pruned" and ctx.get_stat("diameter_bound_pass") == (f32 if fit else 0), (case, f32)
                i, j = ctx.get_stat("diameter_arg_i"), ctx.get_stat("diameter_arg_j")
                assert dist_seq(emb[i - 1], emb[j - 1])[0] == exp, (case, f32, opt, i, j)
    finally:
        ctx.set_option("diameter", 0)
        ctx.set_option("diameter_f32", 2)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_embedding_gives_the_reference_nan(ctx, bad):
    """The reference has no assert on the embedding's values (wGCL's asserts are about sizes and the graph), so the contract
    is its own result: extrema() over distances that hold a NaN is (NaN, NaN) (src/divergence.jl:113; Inf - Inf and
    Inf - mean give the NaN for an Inf).  Comparisons with NaN are false, so a kernel that skips those pairs would
    return the finite maximum of the others: `hi` must be NaN, and the calls must return."""
    from cge.jl_amd import api, synth

    g = synth.abcd_like(3000, 30000, 10, 32, seed=7)
    x = np.array(g["embedding"])
    x[5, 2] = bad
    x[1234, 30] = bad
    emb = np.asfortranarray(x)
    _load(ctx, emb)
    hi, ai, aj = ctx.max_pair_dist()
    assert np.isnan(hi) and (ai, aj) == (1, 1)
    v2l = np.arange(3000) % 60 + 1
    _, ran, _, _ = ctx.diameter_bounds_test(v2l, 60, np.arange(60) % 40 + 1, 40, 2)
    assert ran == 0  # a non-finite centred value is unfit for the low-precision passes
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], emb)
    try:
        ctx.score(g["clusters"], 60, 4, "rss", seed=3, auc_samples=2000)
    except api.CGEError:
        return  # an error code from an earlier phase is no wrong `hi`
    assert np.isnan(ctx.last_diameter()[0])


# ---------------------------------------------------------------------------------------------------------------
# B3. near-ties
def _antipodal(seed, n, d):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n // 2, d))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return np.concatenate([u, -u]) + (3.0 + rng.random(d))


def _polygon(seed, n=2000, d=32):
    rng = np.random.default_rng(seed)
    t = 2 * np.pi * np.arange(n) / n
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return np.stack([np.cos(t), np.sin(t)], 1) @ Q[:2] + rng.standard_normal(d)


def _clusters(seed, d, m=300):
    rng = np.random.default_rng(seed)
    dirn = rng.standard_normal(d)
    dirn /= np.linalg.norm(dirn)
    c = rng.standard_normal((5, d))
    c[0] = -40.0 * dirn + rng.random(d)
    c[1] = 40.0 * dirn + rng.random(d)
    parts = []
    for q in range(5):
        if q < 2:  # 300 copies of one point, each moved by one ulp in one coordinate
            P = np.repeat(c[q][None], m, 0)
            k, up = rng.integers(0, d, m), rng.integers(0, 2, m) * 2 - 1
            P[np.arange(m), k] = np.nextafter(P[np.arange(m), k], np.inf * up)
        else:
            P = c[q] + rng.standard_normal((m, d))
        parts.append(P)
    X = np.concatenate(parts)
    return X[rng.permutation(len(X))]


def _lattice(seed, n=1500, d=5):
    return np.random.default_rng(seed).integers(-8, 9, (n, d)).astype(np.float64)


def emulate_gram_ranking(X):
    """What the library did before it evaluated near-ties: centre, rank by r_i + r_j - 2 X X^T in fp64, take dist() of the
    arg-max pair.  (CPU only; used to choose the inputs below, see the docstring of test_near_ties_keep_the_bits_of_hi.)"""
    Xc = X - X.mean(0)
    r = np.einsum("ij,ij->i", Xc, Xc)
    V = r[:, None] + r[None, :] - 2.0 * (Xc @ Xc.T)
    iu = np.triu_indices(len(X), 1)
    k = int(np.argmax(V[iu]))
    return float(dist_seq(X[iu[0][k]], X[iu[1][k]])[0])


NEAR_TIES = ([("antipodal", s, 1500, d) for d in (2, 5, 32, 128, 200) for s in range(8)]
             + [("antipodal", s, 6000, d) for d in (2, 5, 32, 128, 200) for s in (5, 6)]
             + [("polygon", s, 2000, 32) for s in range(8)]
             + [("clusters", s, 1500, d) for d in (16, 64, 200) for s in range(8)]
             + [("lattice", s, 1500, 5) for s in range(3)])


@pytest.mark.parametrize("family,seed,n,d", NEAR_TIES)
def test_near_ties_keep_the_bits_of_hi(ctx, orc, family, seed, n, d):
    """`hi` == orc.max_pair_dist bit for bit, and the returned pair attains it under dist()'s arithmetic, where many pairs
    lie within a few ulp of the maximum: brute force, its three-part sharded form, and `score` with diameter = 1 and 2.

    The inputs were chosen on the CPU with emulate_gram_ranking (seeds 0..7; "k of 8" = the emulation's value differs from
    orc.max_pair_dist in k seeds, by one ulp each time):
      antipodal (n/2 unit vectors and their negatives + an offset of 3..4 per column; all n/2 antipodal pairs tie exactly in
        real arithmetic), n = 1500: d = 2: 2 of 8, d = 5: 4 of 8, d = 32: 1 of 8, d = 128: 1 of 8, d = 200: 6 of 8;
        n = 6000, d = 32: 1 of 8 (two seeds of each d run here: the oracle is O(n^2 d));
      polygon (regular 2000-gon in a random plane of R^32): 4 of 8;
      clusters (five clusters, the two farthest 300 copies of one point each moved one ulp in one coordinate):
        d = 16: 4 of 8, d = 64: 5 of 8, d = 200: 3 of 8  (axis-aligned cluster centres at d = 16: 0 of 8, not used);
      lattice (integers in -8..8): 0 of 8 -- both arithmetics are exact, any tied pair has the same bits; it guards the tie
        order "smallest (i, j)" of reduce_best and had to pass before near-ties were evaluated.
    The same antipodal points with radii 1 + k 2^-50 (and 2^-52; n = 1500, d = 5, 32, 128, 200, and n = 6000, d = 128) never
    made the emulation differ in 8 seeds -- their pairs are separated by 8 ulp of the squared distance, more than the Gram
    formula loses -- so that family is not run.  The matrix instruction adds in another order than numpy, so the seeds on
    which the GPU ranking differed are not these; the mechanism is.

    On an MI355X, with the library as it was before the near-ties were evaluated (arg-max by the Gram value, dist() of that
    one pair), these cases failed with `hi` one ulp low: antipodal 28 of 50, clusters 14 of 24, polygon 8 of 8, lattice 0 of
    3 (profiles/r08_results_ab.txt).  All pass now."""
    from cge.jl_amd import synth

    X = {"antipodal": lambda: _antipodal(seed, n, d), "polygon": lambda: _polygon(seed, n, d),
         "clusters": lambda: _clusters(seed, d), "lattice": lambda: _lattice(seed, n, d)}[family]()
    emb = np.asfortranarray(X)
    assert emb.shape == (n, d)
    exp = orc.max_pair_dist(emb)
    _load(ctx, emb)
    hi, ai, aj = ctx.max_pair_dist()
    assert hi == exp, (hi, exp, (hi - exp) / exp)
    assert 1 <= ai < aj <= n and dist_seq(emb[ai - 1], emb[aj - 1])[0] == exp
    parts = [ctx.max_pair_dist(p, 3) for p in range(3)]
    best = max(parts)
    assert best[0] == exp and dist_seq(emb[best[1] - 1], emb[best[2] - 1])[0] == exp
    g = synth.abcd_like(n, 10 * n, 10, 4, seed=11)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], emb)
    try:
        for opt in (1, 2):
            ctx.set_option("diameter", opt)
            ctx.score(g["clusters"], 40, 4, "rss", seed=3, auc_samples=2000)
            got, path, pairs, tiles = ctx.last_diameter()
            assert got == exp, (opt, got, exp, path, pairs, tiles)
            assert path == ("brute" if opt == 1 else "pruned")
            i, j = ctx.get_stat("diameter_arg_i"), ctx.get_stat("diameter_arg_j")
            assert dist_seq(emb[i - 1], emb[j - 1])[0] == exp, (opt, i, j)
    finally:
        ctx.set_option("diameter", 0)


# ---------------------------------------------------------------------------------------------------------------
# B4. shapes of the brute-force kernel
@pytest.mark.parametrize("n,d", [(2, 3), (17, 200), (127, 129), (128, 512), (129, 1), (3000, 333)])
def test_max_pair_dist_kernel_small_and_wide(ctx, orc, n, d):
    """One partial tile (n < 128), n = 2, d in (128, 512], d = 1; three shards, and seven (more shards than super-blocks:
    the empty ones answer 0)."""
    rng = np.random.default_rng(n + d)
    emb = np.asfortranarray(rng.standard_normal((n, d)) * rng.random(d) + rng.standard_normal(d) * 3)
    _load(ctx, emb)
    exp = orc.max_pair_dist(emb)
    hi, ai, aj = ctx.max_pair_dist()
    assert hi == exp, (hi, exp)
    assert 1 <= ai < aj <= n and dist_seq(emb[ai - 1], emb[aj - 1])[0] == exp
    for nparts in (3, 7):
        parts = [ctx.max_pair_dist(p, nparts)[0] for p in range(nparts)]
        assert max(parts) == exp and min(parts) >= 0.0, (nparts, parts)


def test_max_pair_dist_identical_rows(ctx, orc):
    """All rows equal: hi = 0, and every pair attains it -- the API returns the smallest one, (1, 2)."""
    rng = np.random.default_rng(4)
    emb = np.asfortranarray(np.repeat(rng.standard_normal((1, 7)) + 3.0, 300, axis=0))
    _load(ctx, emb)
    assert orc.max_pair_dist(emb) == 0.0
    assert ctx.max_pair_dist() == (0.0, 1, 2)
