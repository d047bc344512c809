"""cge_link_sample on the device (`pytest -m gpu`): one draw of the random graph the link model is.

The expected set is always built from the device's own values: cge_link_prob over ALL pairs of the draw, and the reference's
uniforms (tests/link_sample_ref.py, pinned to the scalar counter stream by tests/test_link_sample_ref.py) -- or, through the
testing hook, a matrix of uniforms the test supplies.  It is compared with no tolerance: the ids, their order, out_p bit for bit
and n_edges.  The kernel's filter may only cost exact evaluations ("link_sample_survivors"), never change the set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import link_ref as lr
import link_sample_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _model(ctx, c):
    n = len(c["X"])
    e = np.asfortranarray(np.asarray(c["edges"], np.int64).reshape(-1, 2) + 1)
    ctx.set_graph(e, np.ones(len(e)), n)
    ctx.set_embedding(np.asfortranarray(c["X"]))
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fi"], c["directed"])


def _device_p(ctx, n, directed):
    """cge_link_prob of every pair of a draw: (i, j, p), 0-based, sorted by (i, j)."""
    i, j = sr.all_pairs(n, directed)
    return i, j, (ctx.link_prob(i + 1, j + 1) if len(i) else np.zeros(0))


def _same(got, exp, name):
    gi, gj, gp, ne = got
    ei, ej, ep = exp
    assert ne == len(ei), f"{name}: n_edges {ne}, expected {len(ei)}"
    assert len(gi) == len(gj) == len(gp) == ne
    bad = np.flatnonzero((gi - 1 != ei) | (gj - 1 != ej))
    assert len(bad) == 0, f"{name}: row {bad[0]} is ({gi[bad[0]] - 1}, {gj[bad[0]] - 1}), expected ({ei[bad[0]]}, {ej[bad[0]]})"
    assert gp.tobytes() == np.asarray(ep, np.float64).tobytes(), f"{name}: out_p is not link_prob's"


def _tiles(n, directed):
    nt = (n + 127) // 128
    return nt * nt if directed else nt * (nt + 1) // 2


def _check_draw(ctx, n, directed, seed, stream, name, pij=None):
    i, j, p = pij if pij is not None else _device_p(ctx, n, directed)
    exp = sr.sampled(i, j, p, sr.uniform(seed, stream, i, j))
    got = ctx.link_sample(seed, stream, None, True)
    _same(got, exp, name)
    surv = ctx.get_stat("link_sample_survivors")
    assert ctx.get_stat("link_sample_edges") == got[3] and ctx.get_stat("link_sample_tiles") == _tiles(n, directed)
    assert got[3] <= surv <= len(i)
    print(f"  {name}: {got[3]} edges of {len(i)} pairs, {surv} evaluated exactly")
    return got, (i, j, p)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_sample_shapes(ctx, shape):
    n, d, directed = shape
    _model(ctx, sr.shape_case(*shape))
    got, _ = _check_draw(ctx, n, directed, 11, 0, "shape")
    if n >= 127:
        assert (got[2] > 1).any()  # the heavy vertex's pairs are edges whatever u is


@pytest.mark.parametrize("shape", [s for s in sr.SHAPES if s[0] >= 257], ids=sr.shape_id)
def test_sample_shapes_on_a_smaller_grid(ctx, shape):
    """The grid is min(tiles, 2 cus) workgroups that stride over the tiles: on 256 CUs every shape has a workgroup per tile.  Under
    the testing knob test_device_cus a workgroup walks several; the draw is the reference's all the same, row for row and bit for
    bit, and so are the statistics."""
    n, d, directed = shape
    _model(ctx, sr.shape_case(*shape))
    want, _ = _check_draw(ctx, n, directed, 11, 0, "shape")  # (against the reference)
    surv = ctx.get_stat("link_sample_survivors")
    for cus in (1, 2):
        assert _tiles(n, directed) > 2 * cus  # more tiles than workgroups
        ctx.set_option("test_device_cus", cus)
        try:
            got = ctx.link_sample(11, 0, None, True)
        finally:
            ctx.set_option("test_device_cus", 0)
        assert got[3] == want[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3])), cus
        assert ctx.get_stat("link_sample_survivors") == surv and ctx.get_stat("link_sample_tiles") == _tiles(n, directed)


@pytest.mark.parametrize("directed", [False, True], ids=["und", "dir"])
def test_dense_and_empty(ctx, directed):
    n = 300
    X = lr.points(n, 8, 5)
    c = dict(X=X, hi=2 * lr.diameter(X)[0], alpha=2.25, fo=np.full(n, 10.0), fi=np.full(n, 10.0) if directed else None,
             directed=directed, edges=lr.random_edges(n, 4 * n, 5, directed))
    _model(ctx, c)
    i, j, p = _device_p(ctx, n, directed)
    assert (p >= 1).all()  # the base is at least 1/2 and the factors' product 100
    got, _ = _check_draw(ctx, n, directed, 0, 0, "dense", (i, j, p))
    assert got[3] == (n * (n - 1) if directed else n * (n - 1) // 2)
    ctx.link_set_model(2.25, c["hi"], np.zeros(n), np.zeros(n) if directed else None, directed)
    got = ctx.link_sample(0, 0, None, True)
    assert got[3] == 0 and len(got[0]) == 0 and ctx.get_stat("link_sample_survivors") == 0


@pytest.mark.parametrize("clamped", [False, True], ids=["diameter", "clamped"])
@pytest.mark.parametrize("directed", [False, True], ids=["und", "dir"])
def test_every_pair_on_the_threshold(ctx, directed, clamped):
    """Through the hook, u is what the test says: every pair's own p, the double below it, and p (1 +- 1e-13), p (1 +- 1e-9) by
    a random sign matrix.  The filter has to let every such pair through to the exact comparison."""
    n = 300
    _model(ctx, sr.threshold_case(n, directed, clamped))
    i, j, p = _device_p(ctx, n, directed)
    assert (p > 0).sum() > 1000 and (p == 0).any()
    rng = np.random.default_rng(9)

    def run(u, name):
        U = np.zeros((n, n))  # (the diagonal, and an undirected draw's lower triangle, are never read: 0 would be an edge there)
        U[i, j] = u
        got = ctx.link_sample_test(U, directed, None, True)
        _same(got, sr.sampled(i, j, p, u), name)
        return got[3]

    assert run(p, "u = p") == 0
    assert run(np.nextafter(p, 0.0), "u = the double below p") == (p > 0).sum()
    for eps in (1e-13, 1e-9):
        sign = rng.choice([-1.0, 1.0], len(p))
        u = p * (1.0 + sign * eps)
        assert ((u != p) | (p == 0)).all()
        assert run(u, f"u = p (1 +- {eps:g})") == ((sign < 0) & (p > 0)).sum()


# ---- fitted models ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,directed", [("test115", False), ("test115", True), ("abcd2000-l300", False), ("exact300", False)])
def test_sample_of_a_fitted_model(test115, name, directed):
    """link_fit in landmark mode below (20) and above (300) 256 landmarks and in exact mode (the stored-logarithm power); the
    count lies within 6 sqrt(sum p (1 - p)) of sum min(1, p)."""
    from cge.jl_amd import api, synth

    if name == "test115":
        g, land = test115, 20
    elif name == "exact300":
        g, land = synth.abcd_like(300, 3000, 5, 8, seed=51, directed=directed), -1
    else:
        g, land = synth.abcd_like(2000, 20000, 12, 16, seed=52, directed=directed), 300
    c = api.Context(0)
    try:
        c.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
        vec, _ = c.link_fit(g["clusters"], land, forced=4, method="rss", directed=directed, split=False, seed=17, auc_samples=2000)
        assert len(vec) == 7
        n = len(g["vweights"])
        got, (i, j, p) = _check_draw(c, n, directed, 5, 0, name)
        q = np.minimum(p, 1.0)
        mean, sd = q.sum(), np.sqrt((q * (1 - q)).sum())
        print(f"  {name}: expected {mean:.1f} +- {sd:.1f} edges, the graph has {len(g['eweights'])}")
        assert abs(got[3] - mean) <= 6 * sd
        _check_draw(c, n, directed, 5, 1, name + " stream 1", (i, j, p))
    finally:
        c.close()


def test_api_link_sample_draws_on_streams(test115):
    """api.link_sample: one fit, R draws on the streams 0 .. R - 1 -- the same sets as Context.link_sample stream by stream."""
    import torch

    from cge.jl_amd import api

    a = test115
    ei = torch.from_numpy(np.ascontiguousarray((np.asarray(a["edges"]) - 1).T.astype(np.int32))).cuda()  # PyG's edge_index
    comm = torch.from_numpy(np.ascontiguousarray(np.asarray(a["comm"]).ravel() - 1)).cuda()
    emb = torch.from_numpy(np.ascontiguousarray(np.asarray(a["embedding"], dtype=np.float64))).cuda()
    c = api.Context(0)
    try:
        vec, draws = api.link_sample(ei, emb, comm, 20, seed=17, auc_samples=2000, sample_seed=6, samples=3, want_p=True, base=0, ctx=c)
        assert len(vec) == 7 and len(draws) == 3
        for r, dr in enumerate(draws):
            one = c.link_sample(6, r, None, True)
            assert one[3] == dr[3] > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(one[:3], dr[:3]))
        assert draws[0][0].tobytes() != draws[1][0].tobytes() or draws[0][1].tobytes() != draws[1][1].tobytes()
    finally:
        c.close()


# ---- capacity, repeatability, interference, errors ---------------------------------------------------------------------------------
def test_capacity_and_repeatability(ctx):
    from cge.jl_amd import api

    n, d, directed = 257, 16, True
    _model(ctx, sr.shape_case(n, d, directed))
    full = ctx.link_sample(3, 2, None, True)
    cnt = full[3]
    assert cnt > 100
    assert ctx.link_sample(3, 2, 0)[3] == cnt and len(ctx.link_sample(3, 2, 0)[0]) == 0
    # one short: refused, the count reported; the context stays usable
    oi, oj, ne = np.zeros(cnt, np.int64), np.zeros(cnt, np.int64), C.c_int64(-1)
    rc = ctx.L.cge_link_sample(ctx.h, C.c_int64(3), C.c_int64(2), C.c_int64(cnt - 1), api._p(oi), api._p(oj), None, C.byref(ne))
    assert rc == -7 and ne.value == cnt
    msg = ctx.L.cge_last_error(ctx.h).decode()
    assert f"n_edges = {cnt}" in msg and "too small" in msg
    with pytest.raises(api.CGEError):
        ctx.link_sample(3, 2, cnt - 1)
    exact = ctx.link_sample(3, 2, cnt, True)
    again = ctx.link_sample(3, 2, 4 * cnt, True)
    for a, b, c in zip(full[:3], exact[:3], again[:3]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert exact[3] == again[3] == cnt
    nop = ctx.link_sample(3, 2, cnt, False)
    assert nop[2] is None and nop[0].tobytes() == full[0].tobytes() and nop[1].tobytes() == full[1].tobytes()
    other = ctx.link_sample(3, 3, None, True)
    assert other[3] != cnt or other[0].tobytes() != full[0].tobytes() or other[1].tobytes() != full[1].tobytes()
    other = ctx.link_sample(4, 2, None, True)
    assert other[3] != cnt or other[0].tobytes() != full[0].tobytes() or other[1].tobytes() != full[1].tobytes()


def test_other_queries_in_between_change_nothing(ctx):
    n, d, directed = 600, 40, False
    _model(ctx, sr.shape_case(n, d, directed))
    before = ctx.link_sample(1, 0, None, True)
    ctx.link_topk(np.arange(1, 200), 16, True)
    mid = ctx.link_sample(1, 0, None, True)
    ctx.link_rank(np.arange(1, 100), np.arange(2, 101), True)
    after = ctx.link_sample(1, 0, None, True)
    for a, b, c in zip(before[:3], mid[:3], after[:3]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert before[3] == mid[3] == after[3] > 0


def test_argument_errors(ctx):
    from cge.jl_amd import api

    c = sr.shape_case(127, 17, False)
    _model(ctx, c)

    def call(cap, oi, oj, ne):
        return ctx.L.cge_link_sample(ctx.h, C.c_int64(0), C.c_int64(0), C.c_int64(cap), oi, oj, None, ne)

    buf, ne = np.zeros(10 ** 5, np.int64), C.c_int64(-1)
    assert call(-1, api._p(buf), api._p(buf), C.byref(ne)) == -7 and "cap = -1" in ctx.L.cge_last_error(ctx.h).decode()
    assert call(0, None, None, None) == -7  # a NULL n_edges
    assert call(10 ** 5, None, api._p(buf), C.byref(ne)) == -7 and "out_i" in ctx.L.cge_last_error(ctx.h).decode()
    assert call(10 ** 5, api._p(buf), None, C.byref(ne)) == -7
    assert ne.value == -1  # refused before any work
    with pytest.raises(ValueError):
        ctx.link_sample_test(np.zeros((3, 3)))
    ctx.set_collectives(lambda user, b, count, op: 0, 0, 2)  # (refused before the hook is ever called)
    try:
        with pytest.raises(api.CGEError) as e:
            ctx.link_sample(0, 0, 0)
        assert e.value.code == -7 and "collectives" in str(e.value)
    finally:
        ctx.clear_collectives()
    assert ctx.link_sample(0, 0, 0)[3] > 0  # the model survived them
    ctx.set_embedding(np.asfortranarray(c["X"]))  # drops the model
    for f in (lambda: ctx.link_sample(0, 0, 0), lambda: ctx.link_sample_test(np.zeros((127, 127)))):
        with pytest.raises(api.CGEError) as e:
            f()
        assert e.value.code == -7 and "no link model" in str(e.value)


# ---- cge_links.py --sample --------------------------------------------------------------------------------------------------------
def test_cge_links_sample_writes_link_samples_rows(tmp_path, capsys):
    from cge.jl_amd import api

    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    gdir = os.path.join(ROOT, "tests", "golden", "test115")
    raw = api.read_table(f"{gdir}/test.edgelist", column_major=False)[0][:, :2].astype(np.int64)
    base = int(raw.min())
    out = tmp_path / "sample.txt"
    argv = ["-g", f"{gdir}/test.edgelist", "-c", f"{gdir}/test1col.ecg", "-e", f"{gdir}/test_n2v.embedding", "-l", "20", "--seed", "5",
            "--samples-local", "2000", "--sample", str(out), "--sample-seed", "8"]
    assert cge_links.main(argv) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("[")
    si, sj, _, ne = api.default_context().link_sample(8, 0)  # the model main() fitted is still resident
    assert ne > 0
    assert out.read_text() == "".join(f"{a - 1 + base} {b - 1 + base}\n" for a, b in zip(si.tolist(), sj.tolist()))
    assert cge_links.main(argv + ["--rank", str(out)]) == 1  # --sample excludes --rank
