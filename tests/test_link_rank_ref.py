"""CPU tests of cge_link_rank's reference (tests/link_rank_ref.py), of the device's bookkeeping restated in numpy, of
api.link_metrics, of the C-ABI's declaration and of cge_links.py --rank's argument handling.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import link_rank_ref as rr
import link_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_rank_on_a_line_with_ties_and_exclusion():
    """Five points on a line, equal factors, alpha = 1, hi = 4: p(0, c) = 1 - |x_c| / 4 = 0.75, 0.75, 0.5, 0.75 for c = 1 .. 4."""
    X = np.array([[0.0], [1.0], [1.0], [2.0], [-1.0]])
    one = np.ones(5)
    g, t, cand, lo, up = rr.rank(X, 4.0, 1.0, one, None, [0, 0, 0], [1, 3, 1], exclude=False)
    assert g.tolist() == [0, 3, 0] and t.tolist() == [2, 0, 2] and cand.tolist() == [3, 3, 3]  # (the pair given twice: twice the same)
    assert lo.tolist() == [0, 3, 0] and up.tolist() == [2, 3, 2]
    # the edge 0 - 2 takes 2 out of the candidates of 0 -- either orientation when undirected, only 0 -> 2 when directed
    g, t, cand, _, _ = rr.rank(X, 4.0, 1.0, one, None, [0, 0], [1, 3], edges=[(2, 0), (2, 0), (0, 0)], exclude=True)
    assert g.tolist() == [0, 2] and t.tolist() == [1, 0] and cand.tolist() == [2, 2]
    g, t, cand, _, _ = rr.rank(X, 4.0, 1.0, one, one, [0, 0], [1, 3], edges=[(2, 0)], directed=True, exclude=True)
    assert g.tolist() == [0, 3] and t.tolist() == [2, 0] and cand.tolist() == [3, 3]
    # the target is itself a resident neighbour: it stays the question, the other neighbours go
    g, t, cand, _, _ = rr.rank(X, 4.0, 1.0, one, None, [0], [2], edges=[(0, 2), (0, 1)], exclude=True)
    assert (g[0], t[0], cand[0]) == (0, 1, 2)  # candidates 3 (0.5) and 4 (0.75 = p*)
    # two vertices: no candidate at all
    g, t, cand, lo, up = rr.rank(X[:2], 4.0, 1.0, one[:2], None, [0, 1], [1, 0], exclude=False)
    assert g.tolist() == t.tolist() == cand.tolist() == lo.tolist() == up.tolist() == [0, 0]


def test_excluded_counts_are_the_sizes_of_the_neighbour_sets():
    for directed in (False, True):
        e = lr.random_edges(60, 400, 5, directed)
        nb = lr.neighbours(e, 60, directed)
        assert rr.excluded_counts(e, 60, directed).tolist() == [len(s - {v}) for v, s in enumerate(nb)]


def test_shapes_cover_the_issue():
    S = rr.RANK_SHAPES
    assert {s[0] for s in S} == {2, 127, 128, 129, 257, 1000} and {s[1] for s in S} == {1, 16, 17, 40}
    assert {s[2] for s in S} == {1, 127, 128, 129, 300} and {s[3] for s in S} == {1, 63, 64, 65, 300}
    assert {s[4] for s in S} == {False, True} and {s[5] for s in S} == {False, True}
    for s in S:
        c = rr.shape_case(*s)
        assert len(set(c["i"].tolist())) == s[2] and len(c["i"]) == s[2] * s[3] and (c["i"] != c["j"]).all()
        assert c["j"].min() >= 0 and c["j"].max() < s[0]


def test_stress_cases_are_what_they_claim():
    c = rr.stress_cases()
    d = c["duplicated_rows"]
    g, t, cand, _, _ = rr.rank(d["X"], d["hi"], d["alpha"], d["fo"], None, d["i"], d["j"], d["edges"], False, d["exclude"])
    nq = len(d["i"]) // 3
    assert (t[:nq] >= 1).all()  # 105 ties with 5
    assert g[:nq].tolist() == g[nq:2 * nq].tolist() == g[2 * nq:].tolist() and t[:nq].tolist() == t[2 * nq:].tolist()
    z = c["zero_factor"]
    p = lr.prob(z["X"], z["hi"], z["alpha"], z["fo"], None, z["i"], z["j"])
    assert (np.asarray(p[:6], np.float64) == 0).all() and p[6] > 0 and p[7] > 0
    g, t, cand, _, _ = rr.rank(z["X"], z["hi"], z["alpha"], z["fo"], None, z["i"], z["j"], z["edges"], False, True)
    assert g[0] == 0 and t[0] == cand[0]  # a zero query: every candidate ties at 0
    b = c["diameter_pair"]
    p = lr.prob(b["X"], b["hi"], b["alpha"], b["fo"], None, b["i"], b["j"])
    assert p[0] == 0 and p[1] == 0 and p[2] > 0
    for directed in (False, True):
        nbc = c[f"neighbour_targets_dir{int(directed)}"]
        nb = lr.neighbours(nbc["edges"], 300, directed)
        inside = [int(j) in nb[int(i)] for i, j in zip(nbc["i"], nbc["j"])]
        assert any(inside) and (directed is False or not all(inside))  # directed: j -> i alone does not make j a neighbour of i
    h = c["hub"]
    assert (h["i"] == 17).sum() == 999 and set(h["j"][h["i"] == 17].tolist()) == set(range(1000)) - {17}
    k = c["small_hi"]
    assert k["hi"] < lr.diameter(k["X"])[0]
    assert (np.asarray(lr.prob(k["X"], k["hi"], k["alpha"], k["fo"], None, k["i"], k["j"]), np.float64) == 0).any()
    o = c["common_offset"]
    assert (o["X"] ** 2).sum(axis=1).min() > 1e13


# ---- the device's bookkeeping, restated -------------------------------------------------------------------------------------------
def _scheme_against_brute_force(c):
    n = len(c["X"])
    tables = {}

    def values(a):
        if a not in tables:
            tables[a] = lr.prob(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], np.full(n, a), np.arange(n))
        return tables[a]

    g, t, cand, _, _ = rr.rank(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], c["i"], c["j"], c["edges"], c["directed"], c["exclude"])
    gs, ts, cs = rr.scheme_counts(values, n, c["i"], c["j"], c["edges"], c["directed"], c["exclude"])
    assert gs.tolist() == g.tolist() and ts.tolist() == t.tolist() and cs.tolist() == cand.tolist()
    return t


@pytest.mark.parametrize("name", ["duplicated_rows", "zero_factor", "diameter_pair", "neighbour_targets_dir0",
                                  "neighbour_targets_dir1", "small_hi"])
def test_histogram_scheme_equals_the_brute_force_on_cases_with_ties(name):
    c = rr.stress_cases()[name]
    t = _scheme_against_brute_force(c)
    if name in ("duplicated_rows", "zero_factor", "small_hi"):
        assert (t > 0).any()  # exact ties really occur


@pytest.mark.parametrize("shape", [rr.RANK_SHAPES[1], rr.RANK_SHAPES[3], rr.RANK_SHAPES[5]])
def test_histogram_scheme_equals_the_brute_force_on_shapes(shape):
    """Repeated pairs (n = 2: one pair 63 times), 64 pairs a query under directed exclusion, one query with 300 pairs."""
    _scheme_against_brute_force(rr.shape_case(*shape))


# ---- api.link_metrics -------------------------------------------------------------------------------------------------------------
def test_link_metrics_on_hand_worked_ranks():
    from cge.jl_amd import api

    # ranks 1, 3.5 (one above, three level: 1 + 1 + 3 / 2), 11, and a pair without candidates (rank 1)
    m = api.link_metrics([0, 1, 10, 0], [0, 3, 0, 0], [10, 10, 20, 0], ks=(1, 3, 10))
    assert m["mrr"] == pytest.approx((1 + 1 / 3.5 + 1 / 11 + 1) / 4, rel=1e-15)
    assert m["hits@1"] == 0.5 and m["hits@3"] == 0.5 and m["hits@10"] == 0.75
    assert m["mean_rank"] == (1 + 3.5 + 11 + 1) / 4
    assert m["auc"] == pytest.approx((1.0 + (1 - 2.5 / 10) + 0.5) / 3, rel=1e-15)  # the pair with cand = 0 is left out
    assert m["mrr_optimistic"] == pytest.approx((1 + 1 / 2 + 1 / 11 + 1) / 4, rel=1e-15)
    assert m["mrr_pessimistic"] == pytest.approx((1 + 1 / 5 + 1 / 11 + 1) / 4, rel=1e-15)
    assert list(m) == ["mrr", "hits@1", "hits@3", "hits@10", "mean_rank", "auc", "mrr_optimistic", "mrr_pessimistic"]
    assert set(api.link_metrics([0], [0], [5])) == {"mrr", "hits@1", "hits@10", "hits@50", "hits@100", "mean_rank", "auc",
                                                    "mrr_optimistic", "mrr_pessimistic"}
    e = api.link_metrics([0, 2], [0, 0], [0, 0])  # no pair has a candidate: no AUC
    assert np.isnan(e["auc"]) and e["mrr"] == pytest.approx((1 + 1 / 3) / 2)
    assert all(np.isnan(v) for v in api.link_metrics([], [], []).values())
    with pytest.raises(ValueError):
        api.link_metrics([0, 1], [0], [5, 5])


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------
def test_link_rank_is_declared_and_exported():
    from cge.jl_amd import api

    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    assert re.search(r"int cge_link_rank\(cge_ctx \*ctx, const int64_t \*i, const int64_t \*j, int64_t P, int exclude_edges,\s*"
                     r"int64_t \*out_greater /\* P \*/, int64_t \*out_ties /\* P \*/, int64_t \*out_cand /\* P, may be NULL \*/,\s*"
                     r"double \*out_p /\* P, may be NULL \*/\);", hdr)
    assert "greater <= r <= greater + ties" in hdr  # the consistency with cge_link_topk is stated
    assert "#define CGE_ABI_VERSION 1" in hdr  # an addition: the ABI version stays
    L = api.load_library()
    assert hasattr(L, "cge_link_rank")
    assert L.cge_abi_version() == 1
    assert callable(api.Context.link_rank) and callable(api.link_metrics) and callable(api.link_evaluate)


def test_link_rank_refuses_null_arguments_at_the_boundary():
    from cge.jl_amd import api

    L = api.load_library()
    ids, out, p = np.array([1, 2], dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2)
    args = (ids.ctypes.data, ids.ctypes.data, C.c_int64(2), C.c_int(1), out.ctypes.data, out.ctypes.data, out.ctypes.data, p.ctypes.data)
    assert L.cge_link_rank(None, *args) == -7
    assert L.cge_link_rank(None, ids.ctypes.data, ids.ctypes.data, C.c_int64(2), C.c_int(1), out.ctypes.data, out.ctypes.data, None,
                           None) == -7


# ---- cge_links.py -----------------------------------------------------------------------------------------------------------------
def _links():
    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    return cge_links


def test_cge_links_rank_argument_handling(tmp_path):
    cl = _links()
    base = ["-g", "g.edgelist", "-e", "g.emb", "-l", "20"]
    rf = tmp_path / "held_out.txt"
    rf.write_text("0 3\n2 1\n")
    assert cl.rank_args(base) is None
    assert cl.rank_args(base + ["--rank", str(rf)]) == str(rf)
    assert cl.rank_args(base + ["--rank", str(rf), "--keep-edges"]) == str(rf)
    for bad in (["--rank"], ["--rank", "--keep-edges"], ["--rank", "nowhere.txt"], ["--rank", str(rf), "--pairs", str(rf)],
                ["--rank", str(rf), "--queries", str(rf)]):
        with pytest.raises(cl.LinkArgError):
            cl.rank_args(base + bad)
    # link_args returns exactly what it returned, with the new flag present or not
    assert cl.link_args(base) == {"which": "local", "topk": 10, "queries": None, "pairs": None, "exclude": True}
    assert cl.link_args(base + ["--rank", str(rf), "--keep-edges", "--which", "global"]) == {
        "which": "global", "topk": 10, "queries": None, "pairs": None, "exclude": False}
    line = cl.metrics_line({"mrr": 0.5, "hits@1": 0.25, "auc": 1.0})
    assert line == "# mrr=0.5 hits@1=0.25 auc=1.0"
