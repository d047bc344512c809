"""The set-up of an alpha sweep at kernel level (run with -m gpu on an MI355X): everything the per-alpha kernels read, made once
per sweep, through the testing hook cge_sweep_setup_test -- the sweep's own plan_layout, prepare_distances, k_pow_prepare,
k_pow_matrix and edge_degrees -- against tests/sweep_setup_ref.py.  No test here runs a fit or a score.

a  D as k_dist_matrix stores it: dist()'s bits, symmetric, the caller's diagonal;
b  lo, hi over j >= i and the normalised D, with the extrema placed on the diagonal, in the last ragged tile and in a strictly
   upper tile; hi == lo gives numpy's 0 / 0;
c  a non-finite input makes lo, hi and all of D NaN (the contract tests/test_gpu_diameter.py states for `hi`);
d  the relabel: order, inverse, every permuted array and the community tables, element for element;
e  the stored logarithm in its three layouts, its accuracy, and GD from it;
f  the start vectors and TT;  g  the degree pass.

Every comparison is equality of bits -- a NaN equal to any NaN: 0 / 0 and Inf / Inf carry the sign bit on one machine and not on
the other -- but two bounds:

  the logarithm  |Lh + Ll - log2(fl(1 - D))| <= B |log2(fl(1 - D))| against `decimal` at 60 digits.  pow_parts.hpp claims
                 2^-70.  Measured with pow_parts.hpp compiled for the host (the qualifiers defined away, -ffp-contract=off as
                 the library is built) over _accuracy_inputs() below, the 8450 of its 8451 values with fl(1 - D) > 0: the
                 largest relative error is 2^-70.64 (5.42e-22), at fl(1 - D) = 0x1.69f81d4d49964p-1, just above sqrt(1/2)
                 where log2_dd changes its exponent.  That is within the claim, so B = 2^-70.
  the degrees    inexact weights: |got - exact| <= (k - 1) 2^-53 sum|w| for a vertex's k terms, the bound of a sum in any order.
"""
import functools

import numpy as np
import pytest

import sweep_setup_ref as ref

pytestmark = pytest.mark.gpu

B = 2.0 ** -70
NS = [1, 2, 63, 64, 65, 127, 129, 256, 257, 321]
DS = [1, 2, 15, 16, 17, 33]
SPECIALS = [0.0, 2.0 ** -60, 2.0 ** -30, 0.5, 1.0 - 2.0 ** -53, 1.0]


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _same(a, b):
    """The same bits, a NaN equal to any NaN (and to nothing else); -0.0 is not 0.0."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    bits = np.int64 if a.dtype == np.float64 else np.int32
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(bits)[~na] == b.view(bits)[~nb]).all())


# ---------------------------------------------------------------------------------------------------------------
# the inputs
def _problem(kind, N, d):
    """(emb, dist) of one kind; every pair distance of the "normal" rows is a few units."""
    rng = np.random.default_rng(1000 * N + d)
    emb = rng.standard_normal((N, d))
    dist = 0.01 + 0.01 * rng.random(N)  # below every pair distance
    if kind == "offset":  # cancellation in a - b
        emb += 1e4
    elif kind == "scaled":  # columns over sixty binades
        emb *= 2.0 ** rng.integers(-30, 31, d)
    elif kind == "twins":  # an off-diagonal 0, its two rows in different tiles where there are two
        emb[N - 1] = emb[0]
    elif kind == "diag-hi":  # the largest value sits on the diagonal, the smallest too
        dist[N // 2], dist[0] = 1e3, 0.0
    elif kind == "ragged-hi":  # the largest value in the last (ragged) tile column
        emb[N - 1] += 50.0
    elif kind == "upper-hi":  # ... at (0, N - 1): a strictly upper tile from 65 vertices on
        emb[0] -= 40.0
        emb[N - 1] += 40.0
    elif kind == "equal":  # hi == lo
        emb[:] = emb[0]
        dist[:] = 0.0
    elif kind == "specials":  # d = 1: lo = 0 and hi = 1 exactly, so the normalised diagonal IS dist
        assert d == 1
        emb = np.linspace(0.0, 1.0, N)[:, None]
        dist = np.full(N, 0.25)
        dist[: len(SPECIALS)] = SPECIALS
    elif kind == "non-finite":  # one NaN and one Inf in different tiles, a NaN on the diagonal
        emb[3, min(2, d - 1)] = np.nan
        emb[N - 1, d - 1] = np.inf
        dist[N // 2] = np.nan
    else:
        assert kind == "normal"
    return emb, dist


KINDS = ["offset", "scaled", "twins", "diag-hi", "ragged-hi", "upper-hi"]
CASES = [("normal", N, d) for N in NS for d in DS] + [(k, N, d) for k in KINDS for N, d in [(2, 1), (65, 17), (129, 2), (257, 16), (321, 33)]]


@functools.lru_cache(maxsize=None)
def _expected(kind, N, d):
    emb, dist = _problem(kind, N, d)
    with np.errstate(all="ignore"):
        D = ref.dist_matrix(emb, dist)
        lo, hi = ref.extrema_upper(D)
        return emb, dist, D, np.array([lo, hi]), ref.normalised(D, lo, hi)


_got_cache = {}


def _got(ctx, kind, N, d):
    """One hook call per problem, shared by the tests of D, of the extrema and of the start vectors."""
    key = (id(ctx), kind, N, d)
    if key not in _got_cache:
        emb, dist = _problem(kind, N, d)
        _got_cache[key] = ctx.sweep_setup_test(emb, dist, np.ones(N, np.int64), 1, want=("D_raw", "D", "start"))
    return _got_cache[key]


def _accuracy_inputs():
    """The normalised D the accuracy of the logarithm is tested on: the distinct values of one ordinary matrix and the values
    that reach every branch of log2_dd's exponent handling."""
    x = np.unique(_expected("normal", 129, 17)[4])
    s = _expected("specials", 65, 1)[4]
    assert _same(np.diag(s)[: len(SPECIALS)], np.array(SPECIALS))
    return np.unique(np.concatenate([x, np.unique(s)]))


# ---------------------------------------------------------------------------------------------------------------
# a. D as stored
@pytest.mark.parametrize("kind, N, d", CASES)
def test_stored_distances(ctx, kind, N, d):
    emb, dist, D, _, _ = _expected(kind, N, d)
    got = _got(ctx, kind, N, d)["D_raw"]
    assert _same(got, D)
    assert _same(got, got.T.copy())
    assert _same(np.diag(got), dist)
    if kind == "twins" and N > 1:
        assert got[0, N - 1] == 0.0 and got[N - 1, 0] == 0.0


# b. extrema and normalisation
@pytest.mark.parametrize("kind, N, d", CASES)
def test_extrema_and_normalisation(ctx, kind, N, d):
    _, dist, D, lo_hi, Dn = _expected(kind, N, d)
    got = _got(ctx, kind, N, d)
    if N > 1:  # the inputs put the extrema where their names say
        iu = np.triu_indices(N)
        at = lambda v: (iu[0][np.flatnonzero(D[iu] == v)], iu[1][np.flatnonzero(D[iu] == v)])  # noqa: E731
        hi_i, hi_j = at(lo_hi[1])
        if kind == "diag-hi":
            assert (hi_i == hi_j).all() and (at(lo_hi[0])[0] == at(lo_hi[0])[1]).all()
        if kind == "ragged-hi":
            assert (hi_j == N - 1).all()
        if kind == "upper-hi":
            assert (hi_i[0], hi_j[0]) == (0, N - 1)
        if kind == "twins":
            assert lo_hi[0] == 0.0 and (at(0.0)[0] != at(0.0)[1]).all()
    assert _same(got["lo_hi"], lo_hi)
    assert _same(got["D"], Dn)


@pytest.mark.parametrize("kind, N, d", [("normal", 1, 1), ("normal", 1, 17), ("equal", 2, 1), ("equal", 65, 16), ("equal", 257, 33)])
def test_equal_extrema_give_the_nan_of_zero_by_zero(ctx, kind, N, d):
    _, _, _, lo_hi, Dn = _expected(kind, N, d)
    assert lo_hi[0] == lo_hi[1] and np.isnan(Dn).all()
    got = _got(ctx, kind, N, d)
    assert _same(got["lo_hi"], lo_hi) and _same(got["D"], Dn)


# c. non-finite input
@pytest.mark.parametrize("N, d", [(65, 2), (129, 17), (257, 16), (321, 33)])
def test_non_finite_input_makes_everything_nan(ctx, N, d):
    """extrema() over values that hold a NaN is (NaN, NaN) (src/divergence.jl:92), so the normalisation leaves nothing finite:
    a kernel must not return the finite extrema of the rest.  The hooks only: nothing is fitted on such input."""
    emb, dist, D, lo_hi, Dn = _expected("non-finite", N, d)
    assert np.isnan(lo_hi).all() and np.isnan(Dn).all() and np.isfinite(D).sum() > N * N // 2
    got = _got(ctx, "non-finite", N, d)
    assert _same(got["D_raw"], D)
    assert np.isnan(got["lo_hi"]).all()
    assert np.isnan(got["D"]).all()
    packed_lo_hi, _ = ctx.packed_gd_test(emb, dist, 1.0, 1)
    assert np.isnan(packed_lo_hi).all()


@pytest.mark.parametrize("where", ["embedding", "diagonal", "last element"])
def test_one_nan_is_enough(ctx, where):
    N, d = 130, 3
    emb, dist = _problem("normal", N, d)
    if where == "embedding":
        emb[129, 1] = np.nan  # the last, two-row tile
    elif where == "diagonal":
        dist[64] = np.nan
    else:
        dist[N - 1] = np.nan  # the last element the extrema read
    got = ctx.sweep_setup_test(emb, dist, np.ones(N, np.int64), 1, want=("D",))
    assert np.isnan(got["lo_hi"]).all() and np.isnan(got["D"]).all()
    assert np.isnan(ctx.packed_gd_test(emb, dist, 1.0, 1)[0]).all()


# ---------------------------------------------------------------------------------------------------------------
# d. the relabel
def _communities(N, C, seed):
    """Ids shuffled over the vertices; id C has exactly one member and, from 5 ids on, id 2 none."""
    rng = np.random.default_rng(seed)
    if C == 2:
        return rng.permutation(np.concatenate([np.ones(N - 1, np.int64), [2]]))
    ids = np.array([q for q in range(1, C + 1) if not (C >= 5 and q in (2, C))])
    comm = np.concatenate([ids, rng.choice(ids, N - ids.size - (C >= 5))])
    if C >= 5:
        comm = np.concatenate([comm, [C]])
    return rng.permutation(comm)


def _graph(N, m, seed, weights="unit"):
    """A directed edge list with a hub that carries half of the edges, self-loops and repeated edges; vertex N - 1 is isolated
    when N > 2, vertex 1 only a source and vertex 2 only a sink when N > 4."""
    rng = np.random.default_rng(seed)
    hi = max(N - 1, 1) if N > 2 else N
    src, dst = rng.integers(0, hi, m), rng.integers(0, hi, m)
    src[: m // 4], dst[m // 4: m // 2] = 0, 0  # the hub: half of all edges leave or enter vertex 0
    src[m // 2: m // 2 + 3] = dst[m // 2: m // 2 + 3]  # self-loops
    src[-3:], dst[-3:] = src[:3], dst[:3]  # repeated edges
    if N > 4:
        dst[dst == 1] = 3
        src[src == 2] = 3
        src[-4], dst[-4], src[-5], dst[-5] = 1, 3, 3, 2
    w = {"unit": None, "dyadic": rng.integers(1, 40, m) / 4.0, "inexact": rng.uniform(0.1, 1.0, m)}[weights]
    return src.astype(np.int32), dst.astype(np.int32), w


def _check_layout(got, emb, dist, vw, comm, C, edges, relabel):
    N = emb.shape[0]
    lay = ref.layout(comm, C, relabel)
    assert got["relabel"] == int(relabel)
    if relabel:
        assert _same(got["order"], lay["order"]) and _same(got["old2new"], lay["old2new"])
    else:  # nothing wrote them
        assert (got["order"] == -1).all() and (got["old2new"] == -1).all()
    p = lay["perm"]
    assert _same(got["emb_rl"], emb[p])
    assert _same(got["vec_rl"][0], dist[p]) and _same(got["vec_rl"][1], vw[p])
    if edges is not None:
        deg_out, deg_in = ref.degrees_sequential(N, *edges)
        assert _same(got["vec_rl"][2], deg_in[p]) and _same(got["vec_rl"][3], deg_out[p])
    else:
        assert np.isnan(got["vec_rl"][2:]).all()
    assert _same(got["comm_rl"], (comm[p] - 1).astype(np.int32))
    for key in ("cm_off", "cm_mem", "cm_pos"):
        assert _same(got[key], lay[key]), key
    assert _same(got["D_raw"], ref.dist_matrix(emb[p], dist[p]))


@pytest.mark.parametrize("N", [256, 257, 321])
@pytest.mark.parametrize("C", [2, 5, 37])
@pytest.mark.parametrize("d", [1, 17, 33])
@pytest.mark.parametrize("mode", ["landmarks", "exact"])
def test_relabel(ctx, N, C, d, mode):
    """A landmark-mode undirected sweep is relabelled from 256 vertices on; an exact-mode one under option bvec_blocks, and not
    without it."""
    emb, dist = _problem("normal", N, d)
    comm = _communities(N, C, N + C + d)
    vw = np.random.default_rng(7).random(N) + 0.5
    edges = _graph(N, 500, N + d, "dyadic")
    assert ref.tiles_apply(comm, C)
    want = ("layout", "D_raw")
    if mode == "landmarks":
        got = ctx.sweep_setup_test(emb, dist, comm, C, vw=vw, landmarks=True, edges=edges, want=want)
        _check_layout(got, emb, dist, vw, comm, C, edges, True)
        return
    got = ctx.sweep_setup_test(emb, dist, comm, C, vw=vw, want=want)
    _check_layout(got, emb, dist, vw, comm, C, None, False)
    ctx.set_option("bvec_blocks", 1)
    try:
        got = ctx.sweep_setup_test(emb, dist, comm, C, vw=vw, edges=edges, want=want)
    finally:
        ctx.set_option("bvec_blocks", 0)
    _check_layout(got, emb, dist, vw, comm, C, edges, True)


@pytest.mark.parametrize("d", [1, 17, 33])
def test_forced_relabel_below_the_tiles(ctx, d):
    N, C = 65, 5
    emb, dist = _problem("normal", N, d)
    comm, vw = _communities(N, C, d), np.arange(N) + 1.0
    edges = _graph(N, 300, d, "unit")
    for directed in (False, True):
        got = ctx.sweep_setup_test(emb, dist, comm, C, vw=vw, directed=directed, force_relabel=True, edges=edges, want=("layout", "D_raw"))
        _check_layout(got, emb, dist, vw, comm, C, edges, True)
    got = ctx.sweep_setup_test(emb, dist, comm, C, vw=vw, edges=edges, want=("layout", "D_raw"))
    _check_layout(got, emb, dist, vw, comm, C, edges, False)


@pytest.mark.parametrize("d", [1, 17])
def test_a_layout_the_tiles_decline_is_left_alone(ctx, d):
    """63 communities of one vertex, an id without a member and one large community: block 0 of the sorted order spans 65 ids."""
    N, C = 321, 65
    comm = np.random.default_rng(d).permutation(np.concatenate([np.arange(1, 64), np.full(N - 63, 65)]))
    assert not ref.tiles_apply(comm, C) and N >= 256
    emb, dist = _problem("normal", N, d)
    vw = np.arange(N) + 1.0
    got = ctx.sweep_setup_test(emb, dist, comm, C, vw=vw, landmarks=True, want=("layout", "D_raw"))
    _check_layout(got, emb, dist, vw, comm, C, None, False)


# ---------------------------------------------------------------------------------------------------------------
# e. the logarithm
def _log_problem(N):
    """An ordinary matrix: its normalised D holds a 1 (the largest distance), so fl(1 - D) == 0 occurs."""
    emb, dist = _problem("normal", N, 3)
    comm = np.sort(_communities(N, 5, N)) if N >= 8 else np.ones(N, np.int64)  # (sorted: a relabel is the identity)
    return emb, dist, comm, 5


@pytest.mark.parametrize("N", [1, 64, 65, 129, 256, 257, 321])
@pytest.mark.parametrize("landmarks", [False, True])
def test_log_row_major_forms(ctx, N, landmarks):
    emb, dist, comm, C = _log_problem(N)
    Dn = _expected("normal", N, 3)[4]
    whole = ctx.sweep_setup_test(emb, dist, comm, C, landmarks=landmarks, log_form=1, want=("D", "log"))
    upper = ctx.sweep_setup_test(emb, dist, comm, C, landmarks=landmarks, log_form=2, want=("D", "log"))
    assert _same(whole["D"], Dn) and _same(upper["D"], Dn)
    assert (whole["log_form_ran"], upper["log_form_ran"]) == (1, 2) and whole["log_count"] == upper["log_count"] == N * N
    mask = ref.upper_tile_mask(N)
    for key in ("Lh", "Ll"):
        w, u = whole[key].reshape(N, N), upper[key].reshape(N, N)
        assert not np.isnan(w).any() or N == 1
        assert _same(u[mask], w[mask]), key
        assert np.isnan(u[~mask]).all(), key  # exactly the upper tiles are written
    if N > 1:
        zero = (1.0 - Dn) == 0.0
        assert zero.any()
        assert (whole["Lh"].reshape(N, N)[zero] == -np.inf).all() and (whole["Ll"].reshape(N, N)[zero] == 0.0).all()
    # what a sweep of this shape prepares below the fused fit: the upper tiles in landmark mode, the whole matrix in exact mode
    if N < 256:
        auto = ctx.sweep_setup_test(emb, dist, comm, C, landmarks=landmarks, log_form=0, want=("log",))
        assert auto["log_form_ran"] == (2 if landmarks else 1)
        assert _same(auto["Lh"], (upper if landmarks else whole)["Lh"]) and _same(auto["Ll"], (upper if landmarks else whole)["Ll"])


def test_log_of_nan_stays_nan(ctx):
    emb, dist = _problem("non-finite", 65, 2)
    got = ctx.sweep_setup_test(emb, dist, np.ones(65, np.int64), 1, log_form=1, alpha=3.0, want=("log",))
    assert np.isnan(got["Lh"]).all() and (got["Ll"] == 0.0).all() and np.isnan(got["GD"]).all()


@pytest.mark.parametrize("N", [256, 257, 321])
def test_log_tile_blocked_form(ctx, N):
    emb, dist, comm, C = _log_problem(N)
    whole = ctx.sweep_setup_test(emb, dist, comm, C, landmarks=True, log_form=1, want=("log",))
    got = ctx.sweep_setup_test(emb, dist, comm, C, landmarks=True, log_form=3, alpha=3.0, want=("log",))
    assert got["log_form_ran"] == 3 and got["log_count"] == ref.blocked_count(N) == got["Lh"].size
    idx, mask = ref.blocked_index(N), ref.upper_tile_mask(N)
    outside = np.ones(got["log_count"], bool)
    outside[idx[mask]] = False
    assert outside.sum() == ref.blocked_count(N) - mask.sum()
    for key, zero in (("Lh", np.float64(0.0)), ("Ll", np.float32(0.0))):
        assert _same(got[key][idx[mask]], whole[key].reshape(N, N)[mask]), key
        assert _same(got[key][outside], np.full(outside.sum(), zero)), key  # +0.0 outside the matrix
    assert np.isnan(got["GD"]).all()  # k_pow_matrix cannot read this form: the hook leaves GD alone
    auto = ctx.sweep_setup_test(emb, dist, comm, C, landmarks=True, log_form=0, want=("log",))
    assert auto["log_form_ran"] in (2, 3)  # (3 where the fused fit's geometry takes N on this device)
    if auto["log_form_ran"] == 3:
        assert _same(auto["Lh"], got["Lh"]) and _same(auto["Ll"], got["Ll"])


def test_log_accuracy(ctx):
    """|Lh + Ll - log2(fl(1 - D))| <= B |log2(fl(1 - D))| on the device's own parts (the module docstring has B)."""
    for kind, N, d in (("normal", 129, 17), ("specials", 65, 1)):
        emb, dist, _, _, Dn = _expected(kind, N, d)
        got = ctx.sweep_setup_test(emb, dist, np.ones(N, np.int64), 1, log_form=1, want=("D", "log"))
        assert _same(got["D"], Dn)
        x = 1.0 - Dn.ravel()
        _, first = np.unique(x, return_index=True)
        first = first[x[first] > 0.0]
        if kind == "specials":  # every branch: 1 - D of 1, 1 (rounded), 1 - 2^-30, 0.5, 2^-53 and, not measured here, 0
            assert {1.0, 1.0 - 2.0 ** -30, 0.5, 2.0 ** -53} <= set(x[first]) and (x == 0.0).any()
        err = ref.log2_rel_error(x[first], got["Lh"][first], got["Ll"][first])
        print(f"log2 parts, {kind}: {first.size} values, largest relative error 2^{np.log2(max(err.max(), 1e-300)):.1f}")
        assert err.max() <= B, (err.max(), x[first][err.argmax()])
        one = x == 1.0
        assert (got["Lh"][one] == 0.0).all() and (got["Ll"][one] == 0.0).all()


@pytest.mark.parametrize("alpha", [0.25, 3.0, 10.0])
@pytest.mark.parametrize("N", [65, 257])
def test_power_matrix_from_the_stored_logarithm(ctx, N, alpha):
    emb, dist, comm, C = _log_problem(N)
    Dn = _expected("normal", N, 3)[4]
    expect = ctx.pow_test(Dn.ravel(), alpha, 1).reshape(N, N)
    mask = ref.upper_tile_mask(N)
    for form, written in ((1, np.ones((N, N), bool)), (2, mask)):
        got = ctx.sweep_setup_test(emb, dist, comm, C, log_form=form, alpha=alpha, want=("log",))
        assert got["log_form_ran"] == form
        assert _same(got["GD"][written], expect[written]) and np.isnan(got["GD"][~written]).all()
        assert not np.isnan(got["GD"][written]).any()


# ---------------------------------------------------------------------------------------------------------------
# f. the start vectors
@pytest.mark.parametrize("N", NS)
def test_start_vectors_undirected(ctx, N):
    got = _got(ctx, "normal", N, 1)
    T1, T2, TT, Tld = ref.start(N)
    assert got["Tld"] == Tld == 64 * -(-N // 64)
    assert _same(got["T1"], T1) and _same(got["T2"], T2) and _same(got["TT"], TT)
    assert _same(got["TT"][0, :N], got["T1"]) and (got["TT"][0, N:] == 0).all() and (got["TT"][1:] == 0).all()


@pytest.mark.parametrize("N", [5, 65, 321])
def test_start_vectors_directed(ctx, N):
    emb, dist = _problem("normal", N, 2)
    src, dst, w = _graph(N, 6 * N, N, "dyadic")
    got = ctx.sweep_setup_test(emb, dist, np.ones(N, np.int64), 1, directed=True, edges=(src, dst, w), want=("start",))
    deg_out, deg_in = ref.degrees_sequential(N, src, dst, w)
    assert deg_in[1] == 0 < deg_out[1] and deg_out[2] == 0 < deg_in[2] and deg_in[N - 1] == deg_out[N - 1] == 0
    assert ((deg_in == 0) != (deg_out == 0)).any()
    T1, T2, TT, Tld = ref.start(N, deg_in, deg_out)
    assert _same(got["deg_in"], deg_in) and _same(got["deg_out"], deg_out)
    assert _same(got["T1"], T1) and _same(got["T2"], T2) and _same(got["TT"], TT) and got["Tld"] == Tld
    assert ((got["T1"] == 0) == (got["deg_in"] == 0)).all() and ((got["T2"] == 0) == (got["deg_out"] == 0)).all()


# ---------------------------------------------------------------------------------------------------------------
# g. the degrees
@pytest.mark.parametrize("N, m", [(2, 40), (65, 1000), (321, 4000)])
@pytest.mark.parametrize("weights", ["unit", "dyadic", "inexact"])
def test_degrees(ctx, N, m, weights):
    src, dst, w = _graph(N, m, N + m, weights)
    assert (src == 0).sum() + (dst == 0).sum() >= m // 2 and (src == dst).any()
    emb, dist = _problem("normal", N, 1)
    got = ctx.sweep_setup_test(emb, dist, np.ones(N, np.int64), 1, edges=(src, dst, w), want=())
    out, inn, star, k_out, k_in = ref.degrees(N, src, dst, w)
    assert _same(got["star"], star)
    if weights != "inexact":
        so, si = ref.degrees_sequential(N, src, dst, w)
        assert _same(got["deg_out"], so) and _same(got["deg_in"], si)
        return
    u = ref.LD(2.0) ** -53
    for g, exact, k in ((got["deg_out"], out, k_out), (got["deg_in"], inn, k_in)):
        bound = np.maximum(k - 1, 0) * u * exact  # (the weights are positive: sum|w| is the sum)
        assert (np.abs(g.astype(ref.LD) - exact) <= bound).all()


# ---------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from cge.jl_amd import api

    emb, dist = _problem("normal", 65, 2)
    comm = np.ones(65, np.int64)

    def refused(*a, **k):
        with pytest.raises(api.CGEError):
            ctx.sweep_setup_test(*a, **k)

    refused(np.zeros((0, 2)), np.zeros(0), np.zeros(0, np.int64), 1)
    refused(np.zeros((3, 0)), np.zeros(3), np.ones(3, np.int64), 1)
    refused(emb, dist, comm * 2, 1)
    refused(emb, dist, comm * 0, 1)
    refused(emb, dist, comm, 1, edges=([0, 65], [1, 2], None))
    refused(emb, dist, comm, 1, edges=([0, 1], [-1, 2], None))
    refused(emb, dist, comm, 1, directed=True)
    refused(emb, dist, comm, 1, log_form=3)  # below 256 vertices
    refused(emb, dist, comm, 1, log_form=4)
    big, bdist = _problem("normal", 321, 1)
    declines = np.concatenate([np.arange(1, 64), np.full(321 - 63, 65)])
    refused(big, bdist, declines, 65, landmarks=True, log_form=3)  # the layout declines the tiles
    for key in ("shard_rows", "shard_ingest"):  # the sharded set-up is tests/test_gpu_two_ranks.py's
        ctx.set_option(key, 1)
        try:
            refused(emb, dist, comm, 1)
        finally:
            ctx.set_option(key, 0)
    ctx.set_option("pow_exp2", 0)
    try:
        for form in (1, 2, 3):
            refused(big, bdist, np.ones(321, np.int64) + (np.arange(321) > 100), 2, landmarks=True, log_form=form)
        got = ctx.sweep_setup_test(emb, dist, comm, 1, log_form=0, alpha=3.0, want=("D", "log"))
        assert got["log_form_ran"] == 0 and got["log_count"] == 0
        assert _same(got["GD"], ctx.pow_test(got["D"].ravel(), 3.0, 0).reshape(65, 65))  # the library pow
    finally:
        ctx.set_option("pow_exp2", 1)
    got = ctx.sweep_setup_test(emb, dist, comm, 1, want=("D",))  # the context is as it was
    assert _same(got["D"], _expected("normal", 65, 2)[4])
