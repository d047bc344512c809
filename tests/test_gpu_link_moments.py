"""cge_link_moments on the device (`pytest -m gpu`): expected degrees, community bins B and V, the sweep's vect_C.

Every output is compared element by element with the long-double reference of tests/link_moments_ref.py under its a-priori bound
(|got - ref| <= c_pair sum f f + |S| 2^-53 sum p_ref, c_pair from the kernel's documented arithmetic); Cobs with numpy.bincount on
integer weights, no tolerance.  Each family prints its worst |got - ref| / bound (DESIGN.md section 4.16 records them)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import link_moments_ref as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
CASES = mr.cases()
_REF = {}


def _ref(name, diag):
    """The reference of a named input, computed once and shared (never modified)."""
    if (name, diag) not in _REF:
        _REF[(name, diag)] = mr.moments(CASES[name], diag)
    return _REF[(name, diag)]


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _resident(ctx, c):
    n = len(c["X"])
    e = np.asfortranarray(np.asarray(c["edges"], np.int64).reshape(-1, 2) + 1)
    ctx.set_inputs(e, c["weights"], np.ones(n), c["comm"], np.asfortranarray(c["X"]))
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fi"] if c["directed"] else None, c["directed"])


def _worst(got, r, keys=("deg_out", "deg_in", "B", "V")):
    """max |got - ref| / bound over the outputs; asserts |got - ref| <= bound element by element."""
    worst = 0.0
    for k in keys:
        g = np.asarray(getattr(got, k), np.float64)
        err = np.abs(g.astype(LD) - r[k]).astype(np.float64)
        b = r["bound"][k]
        assert g.shape == b.shape
        bad = np.flatnonzero(~(err <= b))
        assert len(bad) == 0, f"{k}: {len(bad)} of {len(g)} beyond the bound; first [{bad[0]}] got {g[bad[0]]!r} ref {float(r[k][bad[0]])!r} " \
                              f"err {err[bad[0]]:.3e} bound {b[bad[0]]:.3e}"
        nz = b > 0
        if nz.any():
            worst = max(worst, float((err[nz] / b[nz]).max()))
        assert (g[~nz] == 0).all()  # (an empty bin, a row of zero factors: exactly 0)
    return worst


def _stats(ctx):
    return tuple(ctx.get_stat("link_moments_" + k) for k in ("exact", "fast", "saturated", "tiles"))


def _tiles(n, directed):
    nT = (n + 127) // 128
    return nT * nT if directed else nT * (nT + 1) // 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_against_the_reference(ctx, name):
    c = CASES[name]
    _resident(ctx, c)
    n = len(c["X"])
    r0, r1 = _ref(name, False), _ref(name, True)
    m0 = ctx.link_moments(False)
    st = _stats(ctx)
    m1 = ctx.link_moments(True)
    w0, w1 = _worst(m0, r0), _worst(m1, r1)
    print(f"  {name}: c_pair {r0['c_pair']:.2e} worst ratio {max(w0, w1):.3g}; exact {st[0]} fast {st[1]} saturated {st[2]} tiles {st[3]}")
    assert m0.n_comm == c["C"] and m0.directed == c["directed"] and len(m0.B) == r0["L"]
    assert st[0] + st[1] == r0["pairs"] and st[3] == _tiles(n, c["directed"])
    assert st[2] == r0["saturated"] and ctx.get_stat("link_moments_saturated") == r1["saturated"]
    # Cobs: the sweep's vect_C on integer weights, no tolerance
    assert np.array_equal(m0.C, mr.vect_C(c)) and np.array_equal(m1.C, m0.C)
    # diag = 1 differs from diag = 0 by the self pairs' reference terms, within the two bounds
    for k in ("deg_out", "deg_in", "B", "V"):
        dif = (np.asarray(getattr(m1, k), LD) - np.asarray(getattr(m0, k), LD)) - (r1[k] - r0[k])
        assert (np.abs(dif).astype(np.float64) <= r0["bound"][k] + r1["bound"][k]).all()
    if not c["directed"]:
        assert m0.deg_in is m0.deg_out
    # what the input is there for
    if "near_rows" in name or "small_hi" in name:
        assert st[0] > 0 and st[1] > 0
    else:
        assert st[1] > 0 and st[0] >= 1  # the pair that realises hi (base 0) goes through link_p
    if "zero_factors" in name:
        assert (m0.deg_out[np.asarray(c["fo"]) == 0] == 0).all() and (m0.deg_in[np.asarray(c["fi"]) == 0] == 0).all()
    if "saturated" in name:
        assert st[2] > 1000 and (m0.V < m0.B).any()
    if "empty_community" in name:
        from cge.jl_amd import api

        a, b = api.link_bin_pairs(c["C"], False)
        assert (m0.B[(a == 2) | (b == 2)] == 0).all() and (m0.V[(a == 2) | (b == 2)] == 0).all()


def test_raw_pointers_either_degree_vector_and_no_outputs(ctx):
    """Undirected: deg_out and deg_in are the same vector, either pointer may be given; all outputs NULL returns C alone."""
    c = CASES["n300_boundary_in_tile"]
    _resident(ctx, c)
    n = 300
    a, b, nc = np.zeros(n), np.zeros(n), C.c_int64(-1)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert ctx.L.cge_link_moments(ctx.h, C.c_int(0), p(a), None, None, None, None, C.byref(nc)) == 0
    assert ctx.L.cge_link_moments(ctx.h, C.c_int(0), None, p(b), None, None, None, C.byref(nc)) == 0
    assert np.array_equal(a, b) and a.any() and nc.value == 3
    nc = C.c_int64(-1)
    assert ctx.L.cge_link_moments(ctx.h, C.c_int(1), None, None, None, None, None, C.byref(nc)) == 0 and nc.value == 3


# ---- a function of the inputs alone -------------------------------------------------------------------------------------------------
def test_does_not_depend_on_the_cu_count_or_the_call(ctx):
    """n = 700: 6 work items undirected, 9 directed, on 4 or 16 workgroups under the knob and on all of them without: the same
    arrays, and the same again when the call is repeated."""
    for name in ("n700_shuffled_c7", "n700_shuffled_c7_dir", "n700_pairs_of_vertices", "n300_near_rows", "n300_saturated"):
        _resident(ctx, CASES[name])
        full = ctx.link_moments(True)
        again = ctx.link_moments(True)
        runs = [again]
        for cus in (2, 8):
            ctx.set_option("test_device_cus", cus)
            try:
                runs.append(ctx.link_moments(True))
            finally:
                ctx.set_option("test_device_cus", 0)
        for r in runs:
            for k in ("deg_out", "deg_in", "B", "V", "C"):
                assert np.array_equal(getattr(r, k), getattr(full, k)), (name, k)


# ---- against a draw -----------------------------------------------------------------------------------------------------------------
def test_a_draw_lies_within_five_sigmas(ctx):
    """One unsaturated model (n = 700, C = 3): the per-bin edge counts of cge_link_sample lie within 5 sqrt(V) of B, and each
    vertex's degree within five of its own standard deviation sqrt(sum_j p (1 - p)) from the reference."""
    c = CASES["n700_draw"]
    _resident(ctx, c)
    r = _ref("n700_draw", False)
    assert r["saturated"] == 0
    m = ctx.link_moments(False)
    si, sj, _, ne = ctx.link_sample(seed=11, stream=0)
    si, sj = si - 1, sj - 1
    cnt = np.bincount(mr.bin_index(c["comm"], c["C"], False)[si, sj], minlength=len(m.B))
    z = (cnt - m.B) / np.sqrt(m.V)
    deg = np.bincount(si, minlength=700) + np.bincount(sj, minlength=700)
    P = r["P"].astype(np.float64)
    np.fill_diagonal(P, 0.0)
    sd = np.sqrt((P * (1.0 - P)).sum(1))
    zd = (deg - m.deg_out) / sd
    print(f"  draw: {ne} edges, expected {m.B.sum():.1f}; bins z {np.round(z, 2).tolist()}; degrees max |z| {np.abs(zd).max():.2f}")
    assert (np.abs(z) <= 5).all() and (np.abs(zd) <= 5).all()


# ---- fitted models --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True], ids=["und", "dir"])
@pytest.mark.parametrize("split", [False, True], ids=["whole", "split"])
def test_fitted_exact_mode_reproduces_the_sweeps_divergence(test115, directed, split):
    """land = -1, the model of the best divergence: B with diag = 1 is the sweep's own vect_B at the reported alpha, so B and Cobs
    through cge_js give elements 2-4 of the score (1e-9: what the JS traces are held to against the oracle)."""
    from cge.jl_amd import api

    g = test115
    c = api.Context(0)
    try:
        c.set_option("exact_packed_directed", 1)
        c.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
        vec, _ = c.link_fit(g["clusters"], -1, forced=4, method="rss", directed=directed, split=split, seed=17, auc_samples=500,
                            which="global")
        assert len(vec) == 7
        model = c.link_model()
        assert model["alpha"] == vec[0] and model["directed"] == directed
        m = c.link_moments(True)
        d = api.link_divergence(m.C, m.B, m.n_comm, directed, split, ctx=c)
        print(f"  exact {'dir' if directed else 'und'} split {split}: alpha {vec[0]} score {vec[1:4].tolist()} moments {d}")
        assert abs(d["global"] - vec[1]) <= 1e-9 and abs(d["external"] - vec[2]) <= 1e-9 and abs(d["internal"] - vec[3]) <= 1e-9
    finally:
        c.close()


def test_fitted_landmark_mode(test115):
    """A few dozen landmarks: every output against the reference built from the fetched factors; global_vertex is finite."""
    from cge.jl_amd import api

    g = test115
    c = api.Context(0)
    try:
        c.set_inputs(g["edges"], np.ones(len(g["edges"])), g["vweights"], g["comm"], g["embedding"])
        vec, _ = c.link_fit(g["clusters"], 40, forced=4, method="rss", directed=False, split=False, seed=17, auc_samples=500,
                            which="global")
        assert len(vec) == 7
        model = c.link_model()
        assert model["alpha"] == vec[0] and 20 <= len(model["T_out"]) <= 60
        comm = np.asarray(g["comm"], np.int64).ravel()
        case = dict(X=np.asarray(g["embedding"], np.float64), fo=model["f_out"], fi=model["f_in"], alpha=model["alpha"], hi=model["hi"],
                    directed=False, comm=comm, C=int(comm.max()))
        for diag in (False, True):
            m = c.link_moments(diag)
            w = _worst(m, mr.moments(case, diag))
        gv = api.link_divergence(m.C, m.B, m.n_comm, False, False, ctx=c)["global"]
        print(f"  landmarks {len(model['T_out'])}: alpha {vec[0]} global_sweep {vec[1]} global_vertex {gv} worst ratio {w:.3g}")
        assert np.isfinite(gv) and gv >= 0
    finally:
        c.close()


def test_api_link_moments_on_tensors(test115):
    from cge.jl_amd import api

    g = test115
    c = api.Context(0)
    try:
        ei = (np.asarray(g["edges"]).T - 1).astype(np.int64)
        vec, m = api.link_moments(ei, np.ascontiguousarray(g["embedding"]), np.asarray(g["comm"]).ravel() - 1, 20, seed=17,
                                  auc_samples=500, base=0, ctx=c)
        assert len(vec) == 7 and len(m.deg_out) == 115 and c.link_model()["alpha"] == vec[0]
        again = c.link_moments()
        assert np.array_equal(again.B, m.B) and np.array_equal(again.deg_out, m.deg_out)
        rows = api.link_bins_table(m.B, m.V, m.C, m.n_comm, False)
        assert len(rows) == len(m.B) and all(np.isfinite(r[4]) for r in rows)
    finally:
        c.close()


# ---- errors and lifetime ------------------------------------------------------------------------------------------------------------
def test_errors_and_lifetime(ctx, test115):
    from cge.jl_amd import api

    g = test115
    n = len(g["vweights"])
    one = np.ones(n)

    def raises(msg, fn, *args):
        with pytest.raises(api.CGEError) as e:
            fn(*args)
        assert e.value.code == -7 and msg in str(e.value), str(e.value)

    def raw(diag, ncomm=True):
        nc = C.c_int64()
        return ctx.L.cge_link_moments(ctx.h, C.c_int(diag), None, None, None, None, None, C.byref(nc) if ncomm else None)

    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    raises("no link model", ctx.link_moments)
    ctx.link_set_model(2.0, 10.0, one)
    ok = ctx.link_moments()
    assert ok.n_comm == int(np.asarray(g["comm"]).max()) and ok.B.sum() > 0
    for diag in (2, -1):
        assert raw(diag) == -7 and "diag" in ctx.L.cge_last_error(ctx.h).decode()
        assert np.array_equal(ctx.link_moments().B, ok.B)  # the context is usable after each error, the model survived
    assert raw(0, ncomm=False) == -7
    ctx.set_embedding_view(np.ascontiguousarray(g["embedding"]))  # replaces the embedding: the model goes
    raises("no link model", ctx.link_moments)
    ctx.link_set_model(2.0, 10.0, one)
    ctx.set_collectives(lambda user, buf, count, op: 0, 0, 2)  # (refused before the hook is ever called)
    try:
        raises("collectives", ctx.link_moments)
    finally:
        ctx.clear_collectives()
    assert np.array_equal(ctx.link_moments().B, ok.B)
    # no resident communities: a context that was given a graph and an embedding alone
    c2 = api.Context(0)
    try:
        c2.set_graph(g["edges"], g["eweights"], n)
        c2.set_embedding(g["embedding"])
        c2.link_set_model(2.0, 10.0, one)
        raises("no resident communities", c2.link_moments)
    finally:
        c2.close()


# ---- cge_links.py --moments ---------------------------------------------------------------------------------------------------------
def test_cge_links_moments_prints_link_moments_values(capsys, tmp_path):
    from cge.jl_amd import api

    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    gdir = os.path.join(ROOT, "tests", "golden", "test115")
    bins, degs = str(tmp_path / "bins.txt"), str(tmp_path / "deg.txt")
    argv = ["-g", f"{gdir}/test.edgelist", "-c", f"{gdir}/test1col.ecg", "-e", f"{gdir}/test_n2v.embedding", "-l", "20", "--seed", "5",
            "--samples-local", "2000", "--moments", bins, "--degrees", degs]
    assert cge_links.main(argv) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0].startswith("[") and len(lines) == 2
    c = api.default_context()  # the model main() fitted is still resident
    m = c.link_moments()
    model = c.link_model()
    vec = [float(x) for x in lines[0].strip("[]").split(",")]
    gv = api.link_divergence(m.C, m.B, m.n_comm, False, False, ctx=c)["global"]
    assert lines[1] == cge_links.moments_line(gv, vec[1], model["alpha"], "global") and lines[1].startswith("# global_vertex=")
    assert model["alpha"] == vec[0]  # --moments makes --which default to global
    rows = [ln.split() for ln in open(bins).read().strip().split("\n")]
    want = api.link_bins_table(m.B, m.V, m.C, m.n_comm, False)
    assert len(rows) == len(want)
    for r, w in zip(rows, want):
        assert (int(r[0]), int(r[1])) == w[:2] and [float(x) for x in r[2:]] == [float(x) for x in w[2:]]
    drows = [ln.split() for ln in open(degs).read().strip().split("\n")]
    assert len(drows) == 115 and len(drows[0]) == 3
    assert [float(r[2]) for r in drows] == m.deg_out.tolist()
    assert cge_links.main(argv + ["--auc"]) == 1  # --moments excludes --auc
