"""The reference of cge_link_triangles (tests/link_triangles_ref.py) against itself and against known answers, without a GPU; the
boundary's declaration, export and NULL handling; api.link_clustering_table and cge_links.py's flag on hand-made input."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import link_triangles_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
GRAPHS = tr.graphs()
MODELS = tr.models()


# ---- the model side -------------------------------------------------------------------------------------------------------------------
def test_matrix_form_against_the_triple_loop():
    """n = 23: the two long-double forms agree to a few 2^-64 of the value (both sum at most n^2 non-negative products)."""
    c = tr._model(23, 3, 1.0, 7, scale=1.5)
    Q = tr.model_q(c)
    assert (Q == Q.T).all() and (np.diag(Q) == 0).all() and (Q == 1.0).any() and ((Q > 0) & (Q < 1)).any()
    (t, w), (tl, wl) = tr.expected(Q), tr.expected_loops(Q)
    tol = 23 * 23 * LD(2.0) ** -63
    assert (np.abs(t - tl) <= tol * tl).all() and (np.abs(w - wl) <= tol * wl).all()
    assert (t > 0).all() and (t <= w).all()  # q_jk <= 1: a triangle is a closed wedge


@pytest.mark.parametrize("n", [3, 9, 40])
def test_all_ones_model_is_the_complete_graph(n):
    """Every q = 1: t_i = (n - 1)(n - 2) / 2 = w_i, exactly."""
    Q = tr.model_q(tr.all_ones_model(n))
    assert (Q + np.eye(n) == 1.0).all()
    t, w = tr.expected(Q)
    assert (t == (n - 1) * (n - 2) // 2).all() and (w == t).all()


def test_wedge_form_has_no_cancellation():
    """A row with ONE entry has no wedge: the pair sum gives 0 exactly, where (s1^2 - s2) / 2 in fp64 need not."""
    Q = np.zeros((4, 4))
    Q[0, 1] = Q[1, 0] = 0.1
    Q[1, 2] = Q[2, 1] = 0.3
    t, w = tr.expected(Q)
    assert w[0] == 0 and w[2] == 0 and w[3] == 0 and abs(w[1] - LD(0.1) * LD(0.3)) < 1e-19 and (t == 0).all()


def test_the_bound_scales_with_the_value():
    b = tr.bound(385, np.array([0.0, 1.0, 1e-300], LD))
    assert b[0] == 385.0 ** 2 * 2.0 ** -1073 and b[0] > 0 and abs(b[1] - 393 * 2.0 ** -52) < 1e-20 and b[2] < 1e-312 + 1e-300 * 1e-13


def test_named_models_cover_what_they_claim():
    m = MODELS
    assert sorted(len(c["X"]) for c in m.values())[:6] == [5, 127, 128, 129, 129, 129] and {257, 300, 385} <= {len(c["X"]) for c in m.values()}
    assert {c["X"].shape[1] for c in m.values()} == {3, 8, 130} and {c["alpha"] for c in m.values()} == {0.25, 1.0, 6.25}
    Q = tr.model_q(m["n257_saturated"])
    assert (Q == 1.0).sum() > 1000
    Q = tr.model_q(m["n257_small_hi"])
    off = ~np.eye(257, dtype=bool)
    assert (Q[off] == 0).sum() > 1000 and (Q[off] > 0).sum() > 1000
    Q = tr.model_q(m["n129_zero_factors"])
    assert (Q[0] == 0).all() and (Q[:, 128] == 0).all()
    Q = tr.model_q(m["n129_repeated_rows"])
    assert (Q[0, 60:70] == m["n129_repeated_rows"]["fo"][0] * m["n129_repeated_rows"]["fo"][60:70]).all()  # distance 0: base 1
    t, w = tr.expected(tr.model_q(m["n300_equal_factors"]))
    assert float((t.max() - t.min()) / t.max()) < 1e-12  # all rows alike
    t, _ = tr.expected(tr.model_q(m["n385_heavy_vertex"]))
    assert int(np.argmax(t)) == 200 and t[200] > 20 * np.median(t)


# ---- the graph side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tr.KNOWN))
def test_known_answers(name):
    n, e = GRAPHS[name]
    for fn in (tr.observed_loops, tr.observed):
        tri, wed = fn(e, n)
        assert np.array_equal(tri, tr.KNOWN[name][0]) and np.array_equal(wed, tr.KNOWN[name][1])


def test_a_multigraph_equals_its_simple_graph():
    n, e = GRAPHS["multigraph"]
    _, s = GRAPHS["multigraph_simple"]
    assert len(e) > 2 * len(s) and (e[:, 0] == e[:, 1]).any()
    a, b = tr.observed(e, n), tr.observed(s, n)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() == 3 * 5  # K4's four triangles and one more
    al = tr.observed_loops(e, n)
    assert np.array_equal(al[0], a[0]) and np.array_equal(al[1], a[1])


def test_matrix_count_against_the_triple_loop():
    n, e = GRAPHS["isolated_vertices"]
    a, b = tr.observed(e, n), tr.observed_loops(e, n)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() > 0
    assert (a[1][::5] == 0).all() and (a[0][::5] == 0).all()


def test_named_graphs_cover_what_they_claim():
    n, e = GRAPHS["random_multigraph_n300"]
    assert n == 300 and len(e) == 3000 and (e[:, 0] == e[:, 1]).sum() >= 40
    keys = np.minimum(e[:, 0], e[:, 1]) * 300 + np.maximum(e[:, 0], e[:, 1])
    assert len(np.unique(keys)) < len(keys) - 400
    n, e = GRAPHS["hubs_and_clique_n1200"]
    nb = tr.adjacency(e, n)
    deg = np.array([len(s) for s in nb])
    assert deg[0] >= 1100 and 70 <= deg[1] <= 80
    # the oriented list of the clique's lowest vertex holds the other 89: longer than any lane threshold below that
    rank = np.lexsort((np.arange(n), deg))
    pos = np.empty(n, np.int64)
    pos[rank] = np.arange(n)
    out = np.array([sum(pos[x] > pos[v] for x in nb[v]) for v in range(1100, 1190)])
    assert out.max() >= 89 and (out > 64).sum() > 20


# ---- against draws: the reference alone meets the issue's condition -------------------------------------------------------------------
def test_the_reference_meets_the_draw_condition():
    """64 draws of the n = 120 model on the CPU (tests/link_sample_ref.py's stream): the mean triangle and wedge totals lie within
    five standard errors of the expectation -- well inside: |z| < 2 for both."""
    Q = tr.model_q(tr.draw_model())
    tri, wed = tr.cpu_draws(Q)
    zt, zw = tr.draw_condition(Q, tri, wed)
    print(f"  draws: triangles mean {tri.mean():.2f} z {zt:.2f}; wedges mean {wed.mean():.1f} z {zw:.2f}")
    assert tri.mean() > 20 and abs(zt) < 2 and abs(zw) < 2


# ---- the boundary -------------------------------------------------------------------------------------------------------------------
def test_cge_link_triangles_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    m = re.search(r"int cge_link_triangles\(([^;]*)\);", hdr)
    assert m, "cge_link_triangles is not declared in include/cge_hip.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "tri_exp", "wed_exp", "tri_obs", "wed_obs", "summary[4]"]
    assert re.search(r"#define CGE_ABI_VERSION 1\b", hdr)
    assert "int cge_link_triangles_test(" in open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    from cge.jl_amd import api

    L = api.load_library()
    assert hasattr(L, "cge_link_triangles") and hasattr(L, "cge_link_triangles_test") and L.cge_abi_version() == 1
    jl = open(os.path.join(ROOT, "cge.jl_amd", "julia", "CGE_hip.jl")).read()
    assert ":cge_link_triangles" in jl


def test_a_null_context_or_summary_is_an_argument_error():
    from cge.jl_amd import api

    L = api.load_library()
    s = (C.c_double * 4)()
    assert L.cge_link_triangles(None, None, None, None, None, s) == -7
    assert L.cge_link_triangles_test(None, None, C.c_int64(128)) == -7


# ---- api helpers --------------------------------------------------------------------------------------------------------------------
def test_link_clustering_table_on_hand_made_vectors():
    from cge.jl_amd import api

    te, we = np.array([1.0, 0.5, 0.0, 0.0]), np.array([2.0, 2.0, 0.0, 1.0])
    to, wo = np.array([3, 0, 0, 1]), np.array([6, 1, 0, 1])
    t = api.link_clustering_table(te, we, to, wo, [1.5, 5.0, 4.0, 8.0], comm=[7, 3, 3, 7])
    assert t["c_exp"][:2].tolist() == [0.5, 0.25] and np.isnan(t["c_exp"][2]) and t["c_exp"][3] == 0.0
    assert t["c_obs"][[0, 1, 3]].tolist() == [0.5, 0.0, 1.0] and np.isnan(t["c_obs"][2])
    assert t["transitivity_exp"] == 0.3 and t["transitivity_obs"] == 0.5 and t["triangles_exp"] == 0.5 and t["triangles_obs"] == 4 / 3
    assert t["communities"].tolist() == [3, 7] and t["by_community"].tolist() == [[0, 1, 0.5, 2.0], [4, 7, 1.0, 3.0]]
    z = api.link_clustering_table(te, we, to, wo, [0.0, 0.0, 0.0, 0.0])
    assert np.isnan(z["transitivity_exp"]) and np.isnan(z["transitivity_obs"]) and "by_community" not in z


def test_cge_links_clustering_flags():
    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    la = cge_links.link_args(["--clustering", "out.txt"])
    assert la["clustering"] == "out.txt" and "clustering" not in cge_links.link_args([])
    for bad in (["--clustering"], ["--clustering", "o", "--auc"], ["--clustering", "o", "--moments", "m"], ["--clustering", "o", "--sample", "s"]):
        with pytest.raises(cge_links.LinkArgError):
            cge_links.link_args(bad)
    line = cge_links.clustering_line({"transitivity_obs": 0.5, "transitivity_exp": 0.25, "triangles_obs": 4.0, "triangles_exp": 1.5})
    assert line == "# transitivity_obs=0.5 transitivity_exp=0.25 triangles_obs=4.0 triangles_exp=1.5"
