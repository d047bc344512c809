"""CPU tests of cge_link_auc's reference (tests/link_auc_ref.py), of the device's bookkeeping restated in numpy, of the Python
layer's argument checks and api.link_auc_from_counts, of the C-ABI's declaration, of cge_links.py --auc's argument handling, and
the input condition of the statistical GPU test.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import link_auc_ref as ar
import link_ref as lr
import local_score_ref as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _line():
    """Five points on a line, equal factors, alpha = 1, hi = 4: p(a, b) = 1 - |x_a - x_b| / 4."""
    return dict(X=np.array([[0.0], [1.0], [1.0], [2.0], [-1.0]]), hi=4.0, alpha=1.0, fo=np.ones(5), fi=None)


def test_counts_on_a_line_by_hand():
    P = ar.table(_line())
    assert P[0].tolist() == [1.0, 0.75, 0.75, 0.5, 0.75] and P[3, 4] == 0.25 and P[1, 2] == 1.0
    # edges 0-1 (0.75), 3-0 (0.5, listed backwards), 0-1 again, the self loop 2-2 (1.0).  NE: 02 .75, 04 .75, 12 1, 13 .75, 14 .5,
    # 23 .75, 24 .5, 34 .25
    e = [(0, 1), (3, 0), (0, 1), (2, 2)]
    less, ties, pe, nneg = ar.counts(P, e, False)
    assert pe.tolist() == [0.75, 0.5, 0.75, 1.0] and nneg == 8 == ar.n_neg_from_keys(5, e, False)
    assert less.tolist() == [3, 1, 3, 7] and ties.tolist() == [4, 2, 4, 1]
    assert ar.summary(less, ties) == (4.0, 14.0, 11.0)
    assert ar.summary(less, ties, [1.0, 2.0, 0.5, 4.0]) == (7.5, 3 + 2 + 1.5 + 28, 4 + 4 + 2 + 4)
    # directed: only i -> j is resident; (1, 0), (0, 3) are negatives now, 20 ordered pairs minus the two distinct non-loop keys
    less, ties, pe, nneg = ar.counts(P, e, True)
    assert nneg == 18 == ar.n_neg_from_keys(5, e, True)
    assert less.tolist() == [2 * 3 + 1, 2 * 1, 2 * 3 + 1, 2 * 7 + 2] and ties.tolist() == [2 * 4 + 1, 2 * 2 + 1, 2 * 4 + 1, 2]


def test_negatives_follow_the_samplers_rule():
    """cge_draw_samples rejects a candidate (min, max) that a row joins in either orientation (directed: the ordered pair)."""
    for directed in (False, True):
        e = lr.random_edges(60, 400, 5, directed)
        nb = lr.neighbours(e, 60, directed)
        mask = ar.negatives_mask(60, e, directed)
        for i in range(60):
            for j in range(60):
                expect = i != j and j not in nb[i] and (directed or i < j)
                assert mask[i, j] == expect
        assert mask.sum() == ar.n_neg_from_keys(60, e, directed)


def test_shapes_and_cases_cover_the_issue():
    S = ar.AUC_SHAPES
    assert {s[0] for s in S} == {2, 129, 300, 1000} and {s[1] for s in S} == {1, 5, 32, 130} and {s[3] for s in S} == {False, True}
    for n in (129, 300, 1000):
        ms = [s[2] for s in S if s[0] == n]
        assert min(ms) == n - 1 and max(ms) >= 8 * n
    c = ar.shape_case(*S[5])
    e = c["edges"]
    assert (e[1] == e[0]).all() and (e[2] == e[0][::-1]).all() and e[3][0] == e[3][1]  # a repeated row, its mirror, a self loop
    assert np.log10(c["fo"].max() / c["fo"].min()) > 2.5  # three decades
    st = ar.stress_cases()
    assert set(st) == {"ties_between_positives_and_negatives", "equal_factors", "zero_factor", "small_hi_dir0", "small_hi_dir1",
                       "complete", "complete_directed", "star", "alpha_0.25", "alpha_10.0"}
    assert ar.n_neg_from_keys(40, st["complete"]["edges"], False) == 0 == ar.n_neg_from_keys(40, st["complete_directed"]["edges"], True)
    assert st["small_hi_dir0"]["hi"] < lr.diameter(st["small_hi_dir0"]["X"])[0]
    assert (st["star"]["edges"][:, 0] == 17).all() and len(st["star"]["edges"]) == 299


def test_stress_cases_are_what_they_claim():
    st = ar.stress_cases()
    c = st["ties_between_positives_and_negatives"]
    P = ar.table(c)
    less, ties, pe, _ = ar.counts(P, c["edges"], False)
    assert (c["edges"][-2] == [5, 7]).all() and ties[-2] >= 3  # (105, 7), (5, 107), (105, 107)
    assert P[5, 7] == P[105, 7] == P[5, 107] == P[105, 107]
    z = st["zero_factor"]
    less, ties, pe, nneg = ar.counts(ar.table(z), z["edges"], False)
    assert (pe[-3:] == 0).all() and (less[-3:] == 0).all() and (ties[-3:] > 100).all()  # positives and negatives level at 0
    k = st["small_hi_dir0"]
    less, ties, pe, _ = ar.counts(ar.table(k), k["edges"], False)
    assert (pe == 0).any() and (pe > 0).any()


# ---- the device's bookkeeping, restated -------------------------------------------------------------------------------------------
def _scheme_equals_brute_force(c, nparts=(1,)):
    P = ar.table(c)
    n = len(P)
    less, ties, pe, nneg = ar.counts(P, c["edges"], c["directed"])
    assert nneg == ar.n_neg_from_keys(n, c["edges"], c["directed"])
    ntiles = len(ar.tile_positions(n, c["directed"]))
    for k in nparts:
        parts = [ar.scheme(P, c["edges"], c["directed"], p, k) for p in range(k)]
        assert sum(p[2] for p in parts) == ntiles
        assert sum(p[0] for p in parts).tolist() == less.tolist() and sum(p[1] for p in parts).tolist() == ties.tolist()
        for p in parts:
            if p[2] == 0:  # a part without tiles returns zeros
                assert not p[0].any() and not p[1].any()
    return less, ties


@pytest.mark.parametrize("name", ["ties_between_positives_and_negatives", "zero_factor", "small_hi_dir1", "complete", "complete_directed",
                                  "star"])
def test_histogram_scheme_equals_the_brute_force_on_cases_with_ties(name):
    c = ar.stress_cases()[name]
    less, ties = _scheme_equals_brute_force(c)
    if name.startswith("complete"):
        assert not less.any() and not ties.any()
    elif name != "star":
        assert (ties > 0).any()  # exact ties really occur


@pytest.mark.parametrize("shape", [ar.AUC_SHAPES[0], ar.AUC_SHAPES[1], ar.AUC_SHAPES[2], ar.AUC_SHAPES[6]])
def test_histogram_scheme_equals_the_brute_force_on_shapes(shape):
    """n = 2 (no negatives, both orientations), a tile and a row, three tile rows with repeated rows and a self loop."""
    _scheme_equals_brute_force(ar.shape_case(*shape))


@pytest.mark.parametrize("directed", [False, True])
def test_parts_add_up_to_the_whole(directed):
    """n = 300: 6 tiles undirected, 9 directed; 2 and 7 parts, and 64 -- more parts than tiles, most of them empty."""
    c = ar.shape_case(300, 5, 600, directed, 11)
    assert len(ar.tile_positions(300, directed)) == (9 if directed else 6)
    _scheme_equals_brute_force(c, nparts=(2, 7, 64))


def test_tile_positions_are_the_walks():
    """One super-block: position = I * 32 + J; beyond 32 tiles a side the super-blocks come row-major, the upper ones alone when
    undirected; every position is distinct."""
    assert ar.tile_positions(300, False) == {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 33, (1, 2): 34, (2, 2): 66}
    assert ar.tile_positions(300, True)[(2, 0)] == 64
    big = ar.tile_positions(33 * 128, False)
    assert big[(0, 32)] == 1024 and big[(32, 32)] == 2048 and len(set(big.values())) == len(big) == 33 * 34 // 2
    bigd = ar.tile_positions(33 * 128, True)
    assert bigd[(0, 32)] == 1024 and bigd[(32, 0)] == 2048 and bigd[(32, 32)] == 3072 and len(set(bigd.values())) == 33 * 33


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_link_auc_from_counts_is_the_long_double_definition():
    from cge.jl_amd import api

    rng = np.random.default_rng(5)
    less, ties = rng.integers(0, 10 ** 12, 1000), rng.integers(0, 10 ** 6, 1000)
    w = rng.random(1000) + 0.5
    nneg = 10 ** 12 + 7
    for ww in (None, w):
        r = api.link_auc_from_counts(less, ties, ww, nneg)
        W, L, Tq = ar.summary(less, ties, ww)
        assert (r["W"], r["L"], r["Tq"]) == (W, L, Tq)
        den = LD(W) * LD(nneg)
        assert r["local_exact"] == float(LD(1) - LD(L) / den) and r["auc"] == float((LD(L) + LD(Tq) / LD(2)) / den)
    # by hand: one edge above 3 of 4 non-edges and level with the fourth
    r = api.link_auc_from_counts([3], [1], None, 4)
    assert r["local_exact"] == 0.25 and r["auc"] == 0.875
    r = api.link_auc_from_counts([0, 0], [0, 0], None, 0)  # a complete graph
    assert np.isnan(r["local_exact"]) and np.isnan(r["auc"]) and r["W"] == 2.0
    with pytest.raises(ValueError):
        api.link_auc_from_counts([1, 2], [1], None, 5)
    with pytest.raises(ValueError):
        api.link_auc_from_counts([1, 2], [1, 1], [1.0], 5)


def test_link_auc_is_declared_and_exported():
    from cge.jl_amd import api

    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    assert re.search(r"int cge_link_auc\(cge_ctx \*ctx, int part, int nparts, int64_t \*out_less /\* m, may be NULL \*/, "
                     r"int64_t \*out_ties /\* m, may be NULL \*/,\s*double \*out_p /\* m, may be NULL \*/, int64_t \*n_neg, "
                     r"double summary\[3\]\);", hdr)
    assert "#define CGE_ABI_VERSION 1" in hdr  # an addition: the ABI version stays
    L = api.load_library()
    assert hasattr(L, "cge_link_auc") and L.cge_abi_version() == 1
    assert callable(api.Context.link_auc) and callable(api.link_auc) and callable(api.link_auc_from_counts)
    jl = open(os.path.join(ROOT, "cge.jl_amd", "julia", "CGE_hip.jl")).read()
    assert ":cge_link_auc" in jl


def test_link_auc_refuses_null_arguments_at_the_boundary():
    from cge.jl_amd import api

    L = api.load_library()
    nneg, summ = C.c_int64(), np.zeros(3)
    assert L.cge_link_auc(None, C.c_int(0), C.c_int(1), None, None, None, C.byref(nneg), summ.ctypes.data) == -7


def test_context_link_auc_checks_its_parts_before_the_library():
    """Context.link_auc raises on part / nparts before it reaches the library (no context is needed to see it)."""
    from cge.jl_amd import api

    class NoLibrary:
        m = 3

    for part, nparts in ((0, 0), (-1, 2), (2, 2), (5, 3)):
        with pytest.raises(ValueError):
            api.Context.link_auc(NoLibrary(), part, nparts)


# ---- cge_links.py -----------------------------------------------------------------------------------------------------------------
def _links():
    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    return cge_links


def test_cge_links_auc_argument_handling(tmp_path):
    cl = _links()
    base = ["-g", "g.edgelist", "-e", "g.emb", "-l", "20"]
    f = tmp_path / "pairs.txt"
    f.write_text("0 3\n")
    assert cl.link_args(base) == {"which": "local", "topk": 10, "queries": None, "pairs": None, "exclude": True}  # as before
    assert cl.link_args(base + ["--auc", "--which", "global"]) == {"which": "global", "topk": 10, "queries": None, "pairs": None,
                                                                    "exclude": True, "auc": True}
    for other in (["--pairs", str(f)], ["--queries", str(f)], ["--rank", str(f)], ["--sample", str(tmp_path / "s.txt")]):
        with pytest.raises(cl.LinkArgError):
            cl.link_args(base + ["--auc"] + other)
    line = cl.auc_line({"local_exact": 0.125, "auc": 0.9375, "n_pos": 613, "n_neg": 5942}, 4711)
    assert line == "# local_exact=0.125 auc=0.9375 pos=613 neg=5942 survivors=4711"


# ---- the input condition of the statistical GPU test ---------------------------------------------------------------------------------
def _fixture_graph(name, test115):
    if name == "test115":
        g = test115
        return np.asarray(g["edges"], np.int64) - 1, np.asarray(g["embedding"], np.float64)
    from cge.jl_amd import synth

    g = synth.abcd_like(2000, 20000, 12, 16, seed=52, directed=False)
    return np.asarray(g["edges"], np.int64) - 1, np.asarray(g["embedding"], np.float64)


@pytest.mark.parametrize("name,seed,S", sorted({(f[0], f[2], f[3]) for f in ar.FITTED}))
def test_the_samplers_draws_of_the_chosen_seeds_are_typical(test115, name, seed, S):
    """tests/test_gpu_link_auc.py holds element 6 of a score -- S sampled (edge, non-edge) pairs of the seed -- to five standard
    deviations of the exact value.  The fitted model exists on the device alone; what the seed decides is the draw, and that is
    checked here: the sampler's reference draw of (seed, stream 0, S) on the fixture's graph, tallied with the strict pos > neg on
    a Chung-Lu model of the same graph and embedding (degree factors d / sqrt(2 m), alpha = 2, hi = the diameter), lies within
    five standard deviations of that model's exact value, brute force over every pair.  The graphs are undirected with unit
    weights, so the estimate is a plain mean."""
    e, X = _fixture_graph(name, test115)
    n, m = len(X), len(e)
    assert (e[:, 0] != e[:, 1]).all()
    deg = np.bincount(e.ravel(), minlength=n).astype(np.float64)
    f = deg / np.sqrt(2.0 * m)
    sq = (X * X).sum(axis=1)
    hi = 1.001 * float(np.sqrt(max((sq[:, None] + sq[None, :] - 2.0 * (X @ X.T)).max(), 0.0)))  # (at least the diameter)
    ii, jj = np.triu_indices(n, 1)
    P = np.zeros((n, n))
    P[ii, jj] = f[ii] * f[jj] * (1.0 - ls.dist(X, ii, jj, hi)) ** 2.0
    P = P + P.T
    less, ties, pe, nneg = ar.counts(P, e, False)
    W, L, Tq = ar.summary(less, ties)
    q = float(LD(1) - LD(L) / (LD(W) * LD(nneg)))
    lo, up = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    keys = set(((lo << 32) | up).tolist())
    pos = ls.draw_pos(seed, 0, S, m)
    ni, nj, _ = ls.draw_neg(seed, 0, S, n, lambda i, j: ((i << 32) | j) in keys, False)
    est = 1.0 - float((P[e[pos, 0], e[pos, 1]] > P[ni, nj]).mean())
    assert 0.0 < q < 0.5
    assert ar.within_sigmas(est, q, S), (est, q, S)
