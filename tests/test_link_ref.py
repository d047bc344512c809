"""CPU tests of the link model's reference (tests/link_ref.py), of the conditions the GPU tests (tests/test_gpu_link.py) rely on,
of the C-ABI's declarations and of cge_links.py's argument handling.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import link_ref as lr
from local_score_ref import dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---- the reference itself --------------------------------------------------------------------------------------------------------
def test_probabilities_are_the_formula_on_exact_inputs():
    """Dyadic inputs: every operation is exact, so the value is known in closed form."""
    X = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 8.0], [3.0, 4.0]])
    fo, fi = np.array([1.0, 2.0, 4.0, 0.5]), np.array([0.5, 1.0, 2.0, 8.0])
    p = lr.prob(X, 16.0, 2.0, fo, fi, [0, 1, 0, 1, 2], [1, 0, 2, 3, 2])  # distances 5, 5, 8, 0 (one point twice), 0 (i == j)
    assert [float(v) for v in p] == [0.6875 ** 2, 2.0 * 0.5 * 0.6875 ** 2, 2.0 * 0.25, 16.0, 8.0]
    assert float(lr.prob(X, 10.0, 2.0, fo, None, [0], [1])[0]) == float(lr.prob(X, 10.0, 2.0, fo, None, [1], [0])[0])  # symmetric
    # a hi below the diameter: the base is clamped, the value is 0 and not a NaN
    assert float(lr.prob(X, 4.0, 2.5, fo, fi, [0], [1])[0]) == 0.0
    assert float(lr.prob(X, 5.0, 2.5, fo, fi, [0], [1])[0]) == 0.0  # the pair attaining a diameter of 5


def test_the_bound_is_what_the_docstring_derives():
    assert lr.BOUND == 6 * 2.0 ** -53 + 4 * 2.0 ** -64 and lr.BOUND < 7e-16


def test_tie_rules_and_order():
    X = np.array([[0.0], [1.0], [1.0], [2.0], [-1.0]])  # 1 and 2 are one point; 1, 2 and 4 are at distance 1 from 0
    J, P, cnt, _ = lr.topk(X, 4.0, 1.0, np.ones(5), None, [0], 3, exclude=False)
    assert J[0].tolist() == [1, 2, 4] and cnt[0] == 3  # equal values: the smaller j first
    assert float(P[0, 0]) == float(P[0, 1]) == float(P[0, 2]) == 0.75
    J, _, _, _ = lr.topk(X, 4.0, 1.0, np.ones(5), None, [0, 0], 2, exclude=False)
    assert J.tolist() == [[1, 2], [1, 2]]  # a repeated query repeats its list


def test_directed_exclusion_and_k_beyond_the_admissible_count():
    X = lr.points(5, 3, 21)
    e = [(0, 1), (2, 3), (3, 2), (4, 0)]
    J, P, cnt, _ = lr.topk(X, lr.diameter(X)[0], 1.5, np.ones(5), np.ones(5), [0, 1, 4], 7, e, directed=True, exclude=True)
    assert 1 not in J[0, : cnt[0]] and cnt[0] == 3   # 0 -> 1 excludes 1 for query 0
    assert 0 in J[1, : cnt[1]] and cnt[1] == 4       # ... and nothing for query 1
    assert 0 not in J[2, : cnt[2]] and cnt[2] == 3   # 4 -> 0
    assert (J[0, cnt[0]:] == -1).all() and (P[0, cnt[0]:] == 0).all()
    Ju, _, cu, _ = lr.topk(X, lr.diameter(X)[0], 1.5, np.ones(5), None, [1, 0], 7, e, directed=False, exclude=True)
    assert 0 not in Ju[0, : cu[0]] and cu[0] == 3 and cu[1] == 2  # undirected: either orientation counts (0-1, 0-4)
    # a query adjacent to every vertex: nothing is left; self loops and repeated edges change nothing
    star = [(0, 1), (0, 2), (3, 0), (0, 4), (0, 4), (0, 0)]
    assert lr.topk(X, 9.0, 1.5, np.ones(5), None, [0], 2, star, False, True)[2][0] == 0
    assert lr.topk(X, 9.0, 1.5, np.ones(5), None, [1], 7, star, False, True)[2][0] == 3  # a leaf keeps the other leaves


@pytest.mark.parametrize("shape", lr.TOPK_SHAPES[1:8:3])
def test_brute_force_agrees_with_a_full_sort(shape):
    c = lr.shape_case(*shape)
    J, P, cnt, vals = lr.topk(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], c["queries"][:20], c["k"], c["edges"], c["directed"],
                              c["exclude"])
    for q, (cand, p) in enumerate(vals):
        js, ps = lr.topk_by_sort(cand, p, c["k"])
        assert cnt[q] == len(js) == min(c["k"], len(cand))
        assert J[q, : cnt[q]].tolist() == js.tolist() and (P[q, : cnt[q]] == ps).all()


# ---- the conditions of the GPU tests ----------------------------------------------------------------------------------------------
def test_shapes_cover_the_issue():
    S = lr.TOPK_SHAPES
    assert {s[0] for s in S} == {2, 127, 128, 129, 257, 1000} and {s[1] for s in S} == {1, 16, 17, 40}
    assert {s[2] for s in S} == {1, 3, 128, 129, 300} and {s[3] for s in S} == {1, 7, 32, 33, 64}
    assert {s[4] for s in S} == {False, True} and {s[5] for s in S} == {False, True}
    c = lr.shape_case(*[s for s in S if s[2] == 300][0])
    assert len(set(c["queries"].tolist())) < 300  # Q = 300 comes with repeats


def test_exact_cases_have_no_near_ties_but_the_intended_ones():
    """Where the GPU test compares ids one by one, neighbours among a query's first k + 1 reference values are equal (ties by
    construction) or more than 2 BOUND apart, so neither the device's rounding nor this reference's can reorder them."""
    cases = lr.stress_cases()
    seen_tie = False
    for name, c in cases.items():
        if not c["exact"]:
            continue
        _, _, _, vals = lr.topk(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], c["queries"], c["k"], c["edges"], c["directed"],
                                c["exclude"])
        for cand, p in vals:
            ps = np.sort(np.asarray(p, LD))[::-1][: c["k"] + 1]
            for a, b in zip(ps[:-1], ps[1:]):
                if a == b:
                    seen_tie = True
                else:
                    assert (a - b) > 2 * lr.BOUND * a, (name, float(a), float(b))
    assert seen_tie


def test_stress_cases_are_what_they_claim():
    c = lr.stress_cases()
    # all factors equal: the reference's order is the nearest-neighbour order
    e = c["equal_factors"]
    J, _, cnt, _ = lr.topk(e["X"], e["hi"], e["alpha"], e["fo"], None, e["queries"][:5], e["k"], exclude=False)
    for q, i in enumerate(e["queries"][:5]):
        others = np.array([j for j in range(len(e["X"])) if j != i])
        dd = dist(e["X"], np.full(len(others), i), others, 1.0)
        assert J[q].tolist() == others[np.lexsort((others, dd))][: e["k"]].tolist()
    # the far heavy vertex is in every list although it is farther than every other returned candidate
    f = c["far_heavy_vertex"]
    J, _, _, _ = lr.topk(f["X"], f["hi"], f["alpha"], f["fo"], None, f["queries"], f["k"], exclude=False)
    assert (J == 399).any(axis=1).all()
    far = dist(f["X"], f["queries"], np.full(len(f["queries"]), 399), 1.0)
    near = dist(f["X"], np.repeat(f["queries"], f["k"]), J.ravel(), 1.0).reshape(J.shape)
    assert (far >= near.max(axis=1)).all()
    # a query with a zero factor: every value is 0 and the smallest admissible ids win
    z = c["zero_factor"]
    J, P, cnt, vals = lr.topk(z["X"], z["hi"], z["alpha"], z["fo"], None, [3], z["k"], z["edges"], False, True)
    assert (P == 0).all() and J[0].tolist() == vals[0][0][: z["k"]].tolist()
    # the common offset really cancels: squared norms of 4e13 against squared distances of about 80
    o = c["common_offset"]
    assert (o["X"] ** 2).sum(axis=1).min() > 1e13 and o["hi"] < 20
    # ascending scores: for query 999 the value grows with the candidate's id
    a = c["ascending_scores"]
    p = lr.prob(a["X"], a["hi"], a["alpha"], a["fo"], None, np.full(999, 999), np.arange(999))
    assert (np.diff(np.asarray(p, np.float64)) > 0).all()
    # k beyond n: five vertices, k = 7
    assert c["k_beyond_n_exclude1"]["k"] > len(c["k_beyond_n_exclude1"]["X"])
    # descending scores: every query's best k = 33 lie in the first candidate tile, and the k-th value is more than twice the
    # largest of every later tile -- so a workgroup that has walked tile 0 holds thresholds that reject the later tiles whole
    # (the filter's margins are relative 1e-12 and a rounding bound of the Gram value: nothing beside a factor 2)
    s = c["descending_scores"]
    assert s["k"] == 33 and s["X"].shape == (1000, 1)
    J, P, cnt, vals = lr.topk(s["X"], s["hi"], s["alpha"], s["fo"], None, s["queries"], s["k"], exclude=False)
    for q, (cand, p) in enumerate(vals):
        assert cnt[q] == 33 and (J[q] < 128).all()
        for t in range(1, 8):
            assert P[q, 32] > 2 * p[cand // 128 == t].max(), (q, t)
    # near threshold: after tile 0 the k-th value of a query is vertex 33's (94's); the marked vertex of tile 2 beats it, that of
    # tile 4 beats the one of tile 2, that of tile 6 the one of tile 4 -- each by more than 2 BOUND in value and by less than
    # 1e-3 in squared distance, so a threshold radius 1e-3 too tight (squared) rejects it; the last one ends the final list
    s = c["near_threshold"]
    _, _, _, vals = lr.topk(s["X"], s["hi"], s["alpha"], s["fo"], None, s["queries"], s["k"], exclude=False)
    for q, (i, kth) in enumerate(((0, 33), (127, 94))):
        cand, p = vals[q]
        chain = [kth] + [v + q for v in lr.NEAR_THRESHOLD_IDS]
        assert [v // 128 for v in chain] == [0, 2, 4, 6]
        d2 = (s["X"][chain, 0] - s["X"][i, 0]) ** 2
        pv = [p[cand == v][0] for v in chain]
        for t in range(3):
            assert pv[t + 1] > pv[t] * (1 + 4 * lr.BOUND) and d2[t] / 1.001 < d2[t + 1] < d2[t]
        js, _ = lr.topk_by_sort(cand, p, 33)
        assert js[-1] == chain[-1] and set(js[:-1].tolist()) <= set(range(128))


@pytest.mark.parametrize("n,nsl", [(8321, 66), (65700, 512)])
def test_merge_cases_have_entries_in_the_late_slices(n, nsl):
    """tests/test_gpu_link.py's merge tests: with the slices they run on (candidate tile J in slice J mod nsl, lane = slice mod 64,
    head = slice // 64) both queries' lists hold entries of heads >= 1 -- at the cap every head of the 8 and a second tile."""
    m = lr.merge_case(n, 90)
    assert m["k"] == 64 and len(m["queries"]) == 2 and m["X"].shape == (n, 3) and (n + 127) // 128 in (66, 514)
    assert m["hi"] >= np.sqrt(((m["X"][:, None, :] - m["X"][None, :4000:40, :]) ** 2).sum(axis=2)).max()  # (a spot check: hi >= distances)
    for i in m["queries"]:
        cand = np.delete(np.arange(n), i)
        js, ps = lr.topk_by_sort(cand, lr.prob(m["X"], m["hi"], m["alpha"], m["fo"], None, np.full(n - 1, i), cand), 64)
        sl = (js // 128) % nsl
        assert (sl >= 64).sum() >= 8 and len(set(sl.tolist())) >= 20
        if nsl == 512:
            assert set((sl // 64).tolist()) == set(range(8)) and (js // 128 >= 512).any()
        assert all(a == b or a - b > 2 * lr.BOUND * a for a, b in zip(ps[:-1], ps[1:]))  # the order is beyond rounding


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------
def test_link_entry_points_are_declared_and_exported():
    from cge.jl_amd import api

    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    assert re.search(r"int cge_link_fit\(cge_ctx \*ctx, const cge_score_args \*args, int which, double out\[7\], int \*out_len, "
                     r"cge_trace \*trace\);", hdr)
    assert re.search(r"int cge_link_set_model\(cge_ctx \*ctx, int directed, double alpha, double hi, const double \*f_out,", hdr)
    assert re.search(r"int cge_link_model_fetch\(cge_ctx \*ctx, int \*directed, double \*alpha, double \*hi, double \*f_out,", hdr)
    assert re.search(r"int cge_link_prob\(cge_ctx \*ctx, const int64_t \*i, const int64_t \*j, int64_t P, double \*out\);", hdr)
    assert re.search(r"int cge_link_topk\(cge_ctx \*ctx, const int64_t \*queries, int64_t Q, int64_t k, int exclude_edges,", hdr)
    assert "#define CGE_LINK_BEST_LOCAL 1" in hdr and "#define CGE_LINK_BEST_GLOBAL 2" in hdr
    assert "#define CGE_ABI_VERSION 1" in hdr  # an addition: the ABI version stays
    L = api.load_library()
    for name in ("cge_link_fit", "cge_link_set_model", "cge_link_model_fetch", "cge_link_prob", "cge_link_topk"):
        assert hasattr(L, name), name
    assert L.cge_abi_version() == 1
    assert api.Context._LINK_WHICH == {"local": 1, "global": 2}


def test_link_entry_points_refuse_null_arguments_at_the_boundary():
    from cge.jl_amd import api

    L = api.load_library()
    out, ids = np.zeros(8), np.ones(4, dtype=np.int64)
    assert L.cge_link_prob(None, ids.ctypes.data, ids.ctypes.data, C.c_int64(4), out.ctypes.data) == -7
    assert L.cge_link_topk(None, ids.ctypes.data, C.c_int64(4), C.c_int64(2), C.c_int(1), ids.ctypes.data, out.ctypes.data,
                           ids.ctypes.data) == -7
    assert L.cge_link_set_model(None, C.c_int(0), C.c_double(1.0), C.c_double(1.0), out.ctypes.data, None, C.c_int64(8)) == -7
    assert L.cge_link_model_fetch(None, None, None, None, None, None, None, None, None) == -7
    assert L.cge_link_fit(None, None, C.c_int(1), out.ctypes.data, None, None) == -7


# ---- cge_links.py -----------------------------------------------------------------------------------------------------------------
def _links():
    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    return cge_links


def test_cge_links_argument_handling(tmp_path):
    cl = _links()
    base = ["-g", "g.edgelist", "-e", "g.emb", "-l", "20"]
    assert cl.link_args(base) == {"which": "local", "topk": 10, "queries": None, "pairs": None, "exclude": True}
    qf = tmp_path / "q.txt"
    qf.write_text("0\n3\n")
    got = cl.link_args(base + ["--which", "global", "--topk", "64", "--queries", str(qf), "--keep-edges"])
    assert got == {"which": "global", "topk": 64, "queries": str(qf), "pairs": None, "exclude": False}
    for bad in (["--which", "best"], ["--topk", "0"], ["--topk", "65"], ["--topk", "many"], ["--topk"], ["--queries", "nowhere.txt"],
                ["--pairs", str(qf), "--queries", str(qf)], ["--which", "local", "--samples-local", "0"]):
        with pytest.raises(cl.LinkArgError):
            cl.link_args(base + bad)
    assert cl.link_args(base + ["--which", "global", "--samples-local", "0"])["which"] == "global"


def test_cge_links_reads_ids_in_the_edge_files_base(tmp_path):
    cl = _links()
    pf = tmp_path / "pairs.txt"
    pf.write_text("0 3\n2 1\n")
    assert cl.read_ids(str(pf), 2, 0, 4).tolist() == [[1, 4], [3, 2]]  # 0-based file ids -> the library's 1-based
    assert cl.read_ids(str(pf), 1, 0, 4).tolist() == [[1], [3]]
    with pytest.raises(cl.LinkArgError):
        cl.read_ids(str(pf), 2, 1, 4)  # a 1-based graph has no vertex 0
    with pytest.raises(cl.LinkArgError):
        cl.read_ids(str(pf), 2, 0, 3)  # vertex 3 of a 0-based graph of three vertices
    bad = tmp_path / "bad.txt"
    bad.write_text("0.5 1\n")
    with pytest.raises(cl.LinkArgError):
        cl.read_ids(str(bad), 2, 0, 4)
