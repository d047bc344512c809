"""cge_link_moments without a GPU: the reference of tests/link_moments_ref.py against plain loops, its identities, its bound; the
boundary's declaration, export and NULL handling; api.link_bins_table and api.link_divergence on hand-made vectors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import link_moments_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
CASES = mr.cases()


def _tiny(directed, seed):
    c = mr._case(9, 3, directed, 0.25 if directed else 3.0, [1, 1, 1, 2, 2, 3, 3, 3, 3], seed, scale=3.0)
    return c


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("diag", [False, True])
def test_reference_against_plain_loops(directed, diag):
    c = _tiny(directed, 40 + directed)
    r = mr.moments(c, diag)
    do, di, B, V = mr.moments_loops(c, diag)
    for got, want in ((r["deg_out"], do), (r["deg_in"], di), (r["B"], B), (r["V"], V)):
        np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-13, atol=1e-15)
    assert (np.asarray(V) > 0).any() and (r["saturated"] > 0 or not diag)  # the self pairs saturate (f up to 3): V really uses q


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("diag", [False, True])
def test_bins_add_up_to_the_degrees(directed, diag):
    """Undirected: every pair i < j is in one bin and in two degrees, a self pair in one bin and once in one degree.  Directed:
    every ordered pair is in one bin, one out-degree and one in-degree."""
    c = _tiny(directed, 50 + directed)
    r = mr.moments(c, diag)
    sB, so, si = r["B"].sum(), r["deg_out"].sum(), r["deg_in"].sum()
    dg = (np.asarray(c["fo"], LD) * np.asarray(c["fi"], LD)).sum() if diag else LD(0)
    if directed:
        assert abs(sB - so) < 1e-15 * float(sB) and abs(so - si) < 1e-15 * float(sB)
    else:
        assert abs(sB - ((so - dg) / 2 + dg)) < 1e-15 * float(sB)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bound_is_positive_and_capped(name):
    c = CASES[name]
    cp = mr.c_pair(np.asarray(c["X"]).shape[1], c["alpha"])
    assert 0.0 < cp <= mr.C_PAIR_CAP
    r = mr.moments(c, True)
    for k in ("deg_out", "deg_in", "B", "V"):
        b = r["bound"][k]
        ref = np.asarray(r[k], np.float64)
        assert (b >= 0).all() and (b[ref > 0] > 0).all() and np.isfinite(b).all()
    assert (r["bound"]["B"] <= cp * float((np.asarray(c["fo"], LD)[:, None] * np.asarray(c["fi"], LD)[None, :]).sum()) * 1.01 + 1e-300).all()
    # the count of saturated pairs is compared exactly on the GPU: no reference value may sit at the threshold
    S = mr.pair_mask(len(c["X"]), c["directed"], True)
    assert np.abs(r["P"][S].astype(np.float64) - 1.0).min() > 1e-7


def test_c_pair_of_the_documented_range():
    """The header promises c below 1e-8 for alpha >= 0.25 and d <= 512."""
    assert max(mr.c_pair(512, a) for a in (0.25, 0.5, 1.0, 3.0, 10.0)) < 1e-8
    assert mr.c_pair(128, 10.0) < 4e-10


def test_named_inputs_cover_what_they_claim():
    c = CASES
    assert sorted(np.bincount(c["n300_boundary_in_tile"]["comm"])[1:]) == [1, 129, 170]
    assert (np.diff(c["n700_shuffled_c7"]["comm"]) < 0).any() and c["n700_shuffled_c7"]["C"] == 7
    assert c["n700_pairs_of_vertices"]["C"] == 350 and c["n300_pairs_of_vertices_dir"]["C"] == 150
    e = c["n129_empty_community"]
    assert e["C"] == 4 and 2 not in e["comm"]
    D = mr.dist64(c["n300_near_rows"]["X"])
    off = ~np.eye(300, dtype=bool)
    assert (D[off] == 0).any() and ((D[off] > 0) & (D[off] < 1e-7)).any()
    assert mr.dist64(c["n300_small_hi_dir"]["X"]).max() > c["n300_small_hi_dir"]["hi"]
    assert mr.moments(c["n300_saturated"])["saturated"] > 1000 and mr.moments(c["n700_draw"])["saturated"] == 0
    assert {np.asarray(v["X"]).shape[1] for v in c.values()} == {3, 64, 130} and {v["alpha"] for v in c.values()} == {0.25, 3.0, 10.0}


# ---- the boundary -------------------------------------------------------------------------------------------------------------------
def test_cge_link_moments_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    m = re.search(r"int cge_link_moments\(([^;]*)\);", hdr)
    assert m, "cge_link_moments is not declared in include/cge_hip.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "diag", "deg_out", "deg_in", "B", "V", "Cobs", "n_comm"]
    from cge.jl_amd import api

    L = api.load_library()
    assert hasattr(L, "cge_link_moments")
    jl = open(os.path.join(ROOT, "cge.jl_amd", "julia", "CGE_hip.jl")).read()
    assert ":cge_link_moments" in jl


def test_a_null_context_is_an_argument_error():
    from cge.jl_amd import api

    L = api.load_library()
    nc = C.c_int64()
    assert L.cge_link_moments(None, C.c_int(0), None, None, None, None, None, C.byref(nc)) == -7


# ---- api helpers --------------------------------------------------------------------------------------------------------------------
def _js(vC, vB, vI=None, internal=True):
    """src/auxilary.jl:34-52 in numpy."""
    p, q = np.asarray(vC, np.float64), np.asarray(vB, np.float64)
    if vI is not None and len(vI):
        sel = np.asarray(vI).astype(bool) == bool(internal)
        p, q = p[sel], q[sel]
    p = (p + 1) / (p.sum() + len(p))
    q = (q + 1) / (q.sum() + len(q))
    m = (p + q) / 2
    return float((p * np.log(p / m) + q * np.log(q / m)).sum() / 2)


def test_link_bin_pairs_is_the_sweeps_layout():
    from cge.jl_amd import api

    L = api.load_library()
    a, b = api.link_bin_pairs(4, False)
    assert [int(L.cge_idx(4, int(x), int(y))) for x, y in zip(a, b)] == list(range(1, 11))
    a, b = api.link_bin_pairs(3, True)
    assert ((a - 1) * 3 + b).tolist() == list(range(1, 10))


def test_link_bins_table_on_hand_made_vectors():
    from cge.jl_amd import api

    B, V, Cv = [4.0, 1.0, 2.0], [4.0, 0.0, 0.0], [10.0, 3.0, 2.0]
    rows = api.link_bins_table(B, V, Cv, 2, False)
    assert rows[0] == (1, 1, 10.0, 4.0, 2.0, 3.0)
    assert rows[1][:5] == (1, 2, 3.0, 1.0, 0.0) and rows[1][5] == np.inf
    assert rows[2] == (2, 2, 2.0, 2.0, 0.0, 0.0)
    rows = api.link_bins_table([1.0, 5.0, 0.5, 2.0], [1.0, 0.0, 0.25, 4.0], [0.0, 1.0, 1.0, 2.0], 2, True)
    assert [r[:2] for r in rows] == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert [r[5] for r in rows] == [-1.0, -np.inf, 1.0, 0.0]
    with pytest.raises(ValueError):
        api.link_bins_table(B, V, Cv, 3, False)


def test_link_divergence_on_hand_made_vectors():
    from cge.jl_amd import api

    Cv, B = np.array([5.0, 1.0, 0.0, 7.0, 2.0, 3.0]), np.array([4.0, 2.0, 1.0, 6.0, 1.0, 4.0])
    r = api.link_divergence(Cv, B, 3, False, False, js=_js)
    assert r == {"global": _js(Cv, B), "external": 0.0, "internal": 0.0}
    r = api.link_divergence(Cv, B, 3, False, True, js=_js)
    vI = np.array([1, 0, 0, 1, 0, 1])  # (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
    assert r["internal"] == _js(Cv, B, vI, True) and r["external"] == _js(Cv, B, vI, False)
    assert r["global"] == (r["internal"] + r["external"]) / 2.0
    Cd, Bd = np.arange(9.0), np.arange(9.0)[::-1].copy()
    r = api.link_divergence(Cd, Bd, 3, True, True, js=_js)
    vI = np.eye(3, dtype=int).ravel()
    assert r["internal"] == _js(Cd, Bd, vI, True) and r["external"] == _js(Cd, Bd, vI, False)
    with pytest.raises(ValueError):
        api.link_divergence(Cv, B, 4, False, False, js=_js)


# ---- cge_links.py --moments ---------------------------------------------------------------------------------------------------------
def test_cge_links_moments_flags():
    import sys

    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    la = cge_links.link_args(["--moments", "bins.txt"])
    assert la["moments"] == "bins.txt" and la["degrees"] is None and la["which"] == "global"
    la = cge_links.link_args(["--moments", "bins.txt", "--degrees", "deg.txt", "--which", "local"])
    assert la["degrees"] == "deg.txt" and la["which"] == "local"
    assert "moments" not in cge_links.link_args([]) and cge_links.link_args([])["which"] == "local"
    for bad in (["--moments"], ["--degrees", "deg.txt"], ["--moments", "b", "--auc"], ["--moments", "b", "--sample", "s"]):
        with pytest.raises(cge_links.LinkArgError):
            cge_links.link_args(bad)
    assert cge_links.moments_line(0.5, 0.25, 3.0, "global") == "# global_vertex=0.5 global_sweep=0.25 alpha=3.0 which=global"
