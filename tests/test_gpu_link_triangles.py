"""cge_link_triangles on the device (`pytest -m gpu`): the matrix Q through the testing hook, expected triangles and wedges against
the long-double reference under the header's a-priori bound, observed triangles and wedges against brute force, no tolerance.

The contract of the model side is stated against Q's entries, which are exact by definition (cge_link_prob's bits, clamped).  So Q
is first held to cge_link_prob bit for bit, and the long-double reference of tests/link_triangles_ref.py is then built from THAT
matrix: what remains between the device's sums and the reference is the summation alone, which the bound
(n + 8) 2^-52 exact + n^2 2^-1073 covers.  Each family prints its worst |got - ref| / bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import link_triangles_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MODELS = tr.models()
GRAPHS = tr.graphs()
_OBS = {}


def _observed(name):
    """The brute-force counts of a named graph, computed once and shared (never modified)."""
    if name not in _OBS:
        n, e = GRAPHS[name]
        _OBS[name] = tr.observed_loops(e, n) if n <= 40 else tr.observed(e, n)
    return _OBS[name]


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _resident(ctx, c):
    n = len(c["X"])
    e = np.asfortranarray(np.asarray(c["edges"], np.int64).reshape(-1, 2) + 1)
    ctx.set_inputs(e, np.ones(len(e)), np.ones(n), np.ones(n, np.int64), np.asfortranarray(c["X"]))
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"])


def _graph_resident(ctx, n, e):
    """A graph alone matters: any embedding and model make the call legal."""
    e1 = np.asfortranarray(np.asarray(e, np.int64).reshape(-1, 2) + 1)
    ctx.set_inputs(e1, np.ones(len(e1)), np.ones(n), np.ones(n, np.int64), np.asfortranarray(np.zeros((n, 2))))
    ctx.link_set_model(1.0, 1.0, np.ones(n))


def _check_q(ctx, n):
    """Q through the hook: cge_link_prob's bits clamped off the diagonal, zero diagonal and padding, symmetric.  Returns Q (n, n)."""
    Qp = ctx.link_triangles_test()
    ld = 128 * (((n + 127) // 128) | 1)
    assert Qp.shape == (ld, ld)
    i, j = np.divmod(np.arange(n * n, dtype=np.int64), n)
    p = ctx.link_prob(i + 1, j + 1).reshape(n, n)
    want = np.minimum(p, 1.0)
    np.fill_diagonal(want, 0.0)
    Q = Qp[:n, :n]
    assert np.array_equal(Q.view(np.uint64), want.view(np.uint64)), f"{int((Q != want).sum())} entries differ from min(cge_link_prob, 1)"
    assert not Qp[n:, :].any() and not Qp[:, n:].any() and np.array_equal(Qp, Qp.T)
    return Q.copy(), int((np.triu(p, 1) > 1.0).sum())


def _check_expected(n, Q, te, we):
    """|got - ref| <= bound element by element, ref from the device's own Q in long double; returns the worst ratio."""
    t, w = tr.expected(Q)
    worst = 0.0
    for name, got, ref in (("tri_exp", te, t), ("wed_exp", we, w)):
        err = np.abs(np.asarray(got, LD) - ref).astype(np.float64)
        b = tr.bound(n, ref)
        bad = np.flatnonzero(~(err <= b))
        assert len(bad) == 0, f"{name}: {len(bad)} of {n} beyond the bound; first [{bad[0]}] got {got[bad[0]]!r} ref {float(ref[bad[0]])!r} " \
                              f"err {err[bad[0]]:.3e} bound {b[bad[0]]:.3e}"
        assert (np.asarray(got)[ref == 0] == 0).all()
        worst = max(worst, float((err / b).max()))
    return worst


def _tiles(n):
    nT = (n + 127) // 128
    return nT * (nT + 1) // 2


# ---- the model side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_q_and_the_expected_counts(ctx, name):
    c = MODELS[name]
    n = len(c["X"])
    _resident(ctx, c)
    Q, sat = _check_q(ctx, n)
    te, we, to, wo, summ = ctx.link_triangles()
    worst = _check_expected(n, Q, te, we)
    print(f"  {name}: worst ratio {worst:.3g}; saturated {sat}; transitivity exp {summ[0] / summ[1]:.4f}")
    assert ctx.get_stat("link_tri_tiles") == _tiles(n) and ctx.get_stat("link_tri_saturated") == sat
    ld = 128 * (((n + 127) // 128) | 1)
    assert ctx.get_stat("link_tri_matrix_bytes") == 8 * ld * ld
    # summary: the long-double sums of the returned arrays, rounded once
    want = [float(np.asarray(x, LD).sum()) for x in (te, we, to, wo)]
    assert summ.tolist() == want
    tri, wed = tr.observed(c["edges"], n)
    assert np.array_equal(to, tri) and np.array_equal(wo, wed)
    if "saturated" in name:
        assert sat > 1000
    if "zero_factors" in name:
        assert (te[c["fo"] == 0] == 0).all() and (we[c["fo"] == 0] == 0).all()
    if "small_hi" in name:
        assert (Q[~np.eye(n, dtype=bool)] == 0).sum() > 1000


@pytest.mark.parametrize("n", [9, 200])
def test_all_ones_model_is_the_complete_graph(ctx, n):
    """Every q = 1: t_i = (n - 1)(n - 2) / 2 = w_i.  Sums of ones in fp64: exact."""
    c = tr.all_ones_model(n)
    _resident(ctx, c)
    te, we, _, _, summ = ctx.link_triangles(graph=False)
    assert (te == (n - 1) * (n - 2) // 2).all() and np.array_equal(te, we)
    assert ctx.get_stat("link_tri_saturated") == n * (n - 1) // 2 and summ[2] == 0 and summ[3] == 0


def _fitted(test115, land):
    from cge.jl_amd import api

    g = test115
    c = api.Context(0)
    c.set_inputs(g["edges"], np.ones(len(g["edges"])), g["vweights"], g["comm"], g["embedding"])
    vec, _ = c.link_fit(g["clusters"], land, forced=4, method="rss", directed=False, split=False, seed=17, auc_samples=500, which="global")
    assert len(vec) == 7
    return c


@pytest.mark.parametrize("land", [40, -1], ids=["landmarks", "exact_exp2"])
def test_fitted_models(test115, land):
    """The fitted landmark model of test115, and an exact-mode fit, whose power is the stored-logarithm form."""
    c = _fitted(test115, land)
    try:
        Q, sat = _check_q(c, 115)
        te, we, to, wo, summ = c.link_triangles()
        worst = _check_expected(115, Q, te, we)
        e = np.asarray(test115["edges"], np.int64).reshape(-1, 2) - 1
        tri, wed = tr.observed(e, 115)
        assert np.array_equal(to, tri) and np.array_equal(wo, wed)
        print(f"  test115 land {land}: worst ratio {worst:.3g}; transitivity observed {summ[2] / summ[3]:.4f} expected {summ[0] / summ[1]:.4f}")
    finally:
        c.close()


# ---- the graph side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_observed_counts(ctx, name):
    n, e = GRAPHS[name]
    _graph_resident(ctx, n, e)
    te, we, to, wo, summ = ctx.link_triangles(model=False)
    tri, wed = _observed(name)
    assert te is None and we is None and ctx.get_stat("link_tri_tiles") == 0 and summ[0] == 0 and summ[1] == 0
    assert np.array_equal(to, tri) and np.array_equal(wo, wed)
    assert summ[2] == tri.sum() and summ[3] == wed.sum()
    if name in tr.KNOWN:
        assert np.array_equal(to, tr.KNOWN[name][0]) and np.array_equal(wo, tr.KNOWN[name][1])
    if name == "multigraph":
        ts, ws = _observed("multigraph_simple")
        assert np.array_equal(to, ts) and np.array_equal(wo, ws)


@pytest.mark.parametrize("base", [0, 1])
def test_ids_in_either_base_through_the_graph_view(ctx, base):
    n, e = GRAPHS["random_multigraph_n300"]
    e = np.concatenate([e, [[0, 299]]])  # (both end ids occur: the base is the file's own)
    ctx.set_graph_view(np.ascontiguousarray((e + base).T), None, n=n, base=base)
    ctx.set_embedding_view(np.zeros((n, 2)))
    ctx.link_set_model(1.0, 1.0, np.ones(n))
    _, _, to, wo, _ = ctx.link_triangles(model=False)
    tri, wed = tr.observed(e, n)
    assert np.array_equal(to, tri) and np.array_equal(wo, wed)


# ---- a function of the inputs alone -------------------------------------------------------------------------------------------------
def test_does_not_depend_on_the_cu_count_or_the_call(ctx):
    """n = 385: six tiles on 4 or 16 workgroups under the knob and on all of them without: identical arrays, and on a repeat."""
    for name in ("n385_heavy_vertex", "n257_saturated"):
        _resident(ctx, MODELS[name])
        full = ctx.link_triangles()
        runs = [ctx.link_triangles()]
        for cus in (2, 8):
            ctx.set_option("test_device_cus", cus)
            try:
                runs.append(ctx.link_triangles())
            finally:
                ctx.set_option("test_device_cus", 0)
        for r in runs:
            for a, b in zip(r, full):
                assert np.array_equal(a, b), name


# ---- errors and skipped work ----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx):
    from cge.jl_amd import api

    c = MODELS["n129_d3"]
    n = 129

    def raises(msg, fn, *args):
        with pytest.raises(api.CGEError) as e:
            fn(*args)
        assert e.value.code == -7 and msg in str(e.value), str(e.value)

    e = np.asfortranarray(c["edges"] + 1)
    ctx.set_inputs(e, np.ones(len(e)), np.ones(n), np.ones(n, np.int64), np.asfortranarray(c["X"]))
    raises("no link model", ctx.link_triangles)
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"])
    ok = ctx.link_triangles()
    assert ctx.get_stat("link_tri_tiles") == 3
    # a NULL summary
    a = np.zeros(n)
    assert ctx.L.cge_link_triangles(ctx.h, a.ctypes.data_as(C.c_void_p), None, None, None, None) == -7
    assert np.array_equal(ctx.link_triangles()[0], ok[0])
    # a directed model
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fo"][::-1].copy(), True)
    raises("directed", ctx.link_triangles)
    raises("directed", ctx.link_triangles_test)
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"])
    # collectives
    ctx.set_collectives(lambda user, buf, count, op: 0, 0, 2)  # (refused before the hook is ever called)
    try:
        raises("collectives", ctx.link_triangles)
    finally:
        ctx.clear_collectives()
    # the hook's leading dimension
    bad = np.zeros((128, 128))
    assert ctx.L.cge_link_triangles_test(ctx.h, bad.ctypes.data_as(C.c_void_p), C.c_int64(128)) == -7
    assert "384" in ctx.L.cge_last_error(ctx.h).decode()
    again = ctx.link_triangles()
    for x, y in zip(again, ok):
        assert np.array_equal(x, y)
    # a NULL half skips its work; one NULL array of a half skips that kernel alone
    summ = np.zeros(4)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    to = np.zeros(n, np.int64)
    assert ctx.L.cge_link_triangles(ctx.h, None, None, p(to), None, p(summ)) == 0
    assert ctx.get_stat("link_tri_tiles") == 0 and summ[0] == 0 and summ[1] == 0 and np.array_equal(to, ok[2]) and summ[3] == ok[4][3]
    we = np.zeros(n)
    assert ctx.L.cge_link_triangles(ctx.h, None, p(we), None, None, p(summ)) == 0
    assert ctx.get_stat("link_tri_tiles") == 0 and np.array_equal(we, ok[1]) and summ[0] == 0 and summ[1] == ok[4][1] and summ[2] == 0
    te = np.zeros(n)
    assert ctx.L.cge_link_triangles(ctx.h, p(te), None, None, None, p(summ)) == 0
    assert ctx.get_stat("link_tri_tiles") == 3 and np.array_equal(te, ok[0]) and summ[1] == 0
    ctx.set_embedding_view(np.ascontiguousarray(c["X"]))  # replaces the embedding: the model goes
    raises("no link model", ctx.link_triangles)


# ---- against draws --------------------------------------------------------------------------------------------------------------------
def test_draws_agree_with_the_expectation(ctx):
    """n = 120, 64 draws of cge_link_sample on the streams 0 .. 63 of seed 2024: the mean total triangle count lies within five
    standard errors (estimated from the draws) of sum tri_exp / 3, the mean wedge count within five of sum wed_exp.  The reference
    alone (tests/test_link_triangles_ref.py, the same stream on the CPU) gives z = -1.00 for triangles and -0.93 for wedges."""
    c = tr.draw_model()
    n = tr.DRAW_N
    _resident(ctx, c)
    _, _, _, _, summ = ctx.link_triangles(graph=False)
    tri, wed = [], []
    for s in range(tr.DRAW_DRAWS):
        si, sj, _, _ = ctx.link_sample(seed=tr.DRAW_SEED, stream=s)
        t, w = tr.observed(np.stack([si - 1, sj - 1], 1), n)
        tri.append(t.sum() // 3)
        wed.append(w.sum())
    tri, wed = np.array(tri, np.float64), np.array(wed, np.float64)
    zt = (tri.mean() - summ[0] / 3) / (tri.std(ddof=1) / np.sqrt(len(tri)))
    zw = (wed.mean() - summ[1]) / (wed.std(ddof=1) / np.sqrt(len(wed)))
    print(f"  draws: triangles mean {tri.mean():.2f} expected {summ[0] / 3:.2f} z {zt:.2f}; wedges mean {wed.mean():.1f} expected {summ[1]:.1f} z {zw:.2f}")
    assert abs(zt) <= 5 and abs(zw) <= 5


# ---- api and cge_links.py -------------------------------------------------------------------------------------------------------------
def test_api_link_clustering_on_tensors(test115):
    from cge.jl_amd import api

    g = test115
    c = api.Context(0)
    try:
        ei = (np.asarray(g["edges"]).T - 1).astype(np.int64)
        comm = np.asarray(g["comm"]).ravel() - 1
        vec, t = api.link_clustering(ei, np.ascontiguousarray(g["embedding"]), comm, 20, seed=17, auc_samples=500, base=0, ctx=c)
        assert len(vec) == 7 and len(t["tri_exp"]) == 115
        again = c.link_triangles()
        assert np.array_equal(again[0], t["tri_exp"]) and np.array_equal(again[2], t["tri_obs"])
        assert t["by_community"].shape == (len(np.unique(comm)), 4) and t["by_community"][:, 0].sum() == t["tri_obs"].sum()
        assert 0 < t["transitivity_exp"] < 1 and 0 < t["transitivity_obs"] < 1
    finally:
        c.close()


def test_cge_links_clustering_prints_link_triangles_values(capsys, tmp_path):
    from cge.jl_amd import api

    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    gdir = os.path.join(ROOT, "tests", "golden", "test115")
    out = str(tmp_path / "clustering.txt")
    argv = ["-g", f"{gdir}/test.edgelist", "-c", f"{gdir}/test1col.ecg", "-e", f"{gdir}/test_n2v.embedding", "-l", "20", "--seed", "5",
            "--samples-local", "2000", "--clustering", out]
    assert cge_links.main(argv) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0].startswith("[") and len(lines) == 2
    c = api.default_context()  # the model main() fitted is still resident
    t = api.link_clustering_table(*c.link_triangles())
    assert lines[1] == cge_links.clustering_line(t) and lines[1].startswith("# transitivity_obs=")
    rows = [ln.split() for ln in open(out).read().strip().split("\n")]
    assert len(rows) == 115 and [int(r[0]) for r in rows] == list(range(1, 116))
    assert [int(r[1]) for r in rows] == t["tri_obs"].tolist() and [int(r[2]) for r in rows] == t["wed_obs"].tolist()
    assert [float(r[3]) for r in rows] == t["tri_exp"].tolist() and [float(r[4]) for r in rows] == t["wed_exp"].tolist()
    assert cge_links.main(argv + ["--auc"]) == 1  # --clustering excludes --auc
