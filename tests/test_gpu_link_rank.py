"""cge_link_rank on the device (`pytest -m gpu`): the exact filtered rank of given pairs among the candidates of their source.

Every case is held to three checks (`_check`):
  1. exactly, against the definition evaluated with the device's own values: cge_link_prob of (i, c) for every c, compared in
     numpy with out_p -- greater, ties and cand equal, no tolerance; out_p is cge_link_prob's value bit for bit;
  2. against the long-double reference (tests/link_rank_ref.py), with the bracket derived there and nothing to choose:
         #{c : p_ref(c) > p*_ref (1 + 2 BOUND)} <= greater,    greater + ties <= #{c : p_ref(c) >= p*_ref (1 - 2 BOUND)};
  3. against top-k: for the queries' lists at k = 33, every listed j at position r has greater <= r <= greater + ties."""
import os
import sys

import numpy as np
import pytest

import link_rank_ref as rr
import link_ref as lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _resident(ctx, X, edges0):
    n = len(X)
    e = np.asfortranarray(np.asarray(edges0, np.int64).reshape(-1, 2) + 1)
    ctx.set_graph(e, np.ones(len(e)), n)
    ctx.set_embedding(np.asfortranarray(X))


def _device_tables(ctx, n, queries):
    """cge_link_prob of (a, c) for every c, per distinct query a (0-based): {a: (n,) values}."""
    qs = np.unique(np.asarray(queries, np.int64))
    vals = ctx.link_prob(np.repeat(qs, n) + 1, np.tile(np.arange(n), len(qs)) + 1).reshape(len(qs), n)
    return {int(a): vals[r] for r, a in enumerate(qs)}


def _brute_on_device_values(ctx, n, i, j, edges0, directed, exclude):
    nbrs = lr.neighbours(edges0, n, directed)
    tables = _device_tables(ctx, n, i)
    masks = {a: rr._admissible_mask(a, n, nbrs, exclude) for a in tables}
    out = np.array([rr.counts_of(tables[int(a)], masks[int(a)], int(b)) for a, b in zip(i, j)], np.int64).reshape(-1, 3)
    return out[:, 0], out[:, 1], out[:, 2], np.array([tables[int(a)][int(b)] for a, b in zip(i, j)])


def _exactly(ctx, n, i, j, edges0, directed, exclude, name):
    """Check 1; returns the device's counts."""
    g, t, cand, p = ctx.link_rank(i + 1, j + 1, exclude)
    assert p.tobytes() == ctx.link_prob(i + 1, j + 1).tobytes(), f"{name}: out_p is not link_prob's"
    gb, tb, cb, pb = _brute_on_device_values(ctx, n, i, j, edges0, directed, exclude)
    assert p.tobytes() == pb.tobytes()
    bad = np.flatnonzero((g != gb) | (t != tb) | (cand != cb))
    assert len(bad) == 0, (f"{name}: {len(bad)} of {len(i)} pairs differ from the definition; first: pair {bad[0]} = "
                           f"({i[bad[0]]}, {j[bad[0]]}) got {(g[bad[0]], t[bad[0]], cand[bad[0]])} "
                           f"expected {(gb[bad[0]], tb[bad[0]], cb[bad[0]])}")
    return g, t, cand, p


def _check(ctx, c, name, topk=True):
    X, n, i, j = c["X"], len(c["X"]), c["i"], c["j"]
    _resident(ctx, X, c["edges"])
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fi"], c["directed"])
    g, t, cand, p = _exactly(ctx, n, i, j, c["edges"], c["directed"], c["exclude"], name)
    nq = len(set(i.tolist()))
    assert ctx.get_stat("link_rank_queries") == nq
    surv = ctx.get_stat("link_rank_survivors")
    assert 0 <= surv <= nq * n
    # 2. the long-double reference's bracket, every pair
    _, _, cr, lo, up = rr.rank(X, c["hi"], c["alpha"], c["fo"], c["fi"], i, j, c["edges"], c["directed"], c["exclude"])
    print(f"  {name}: {len(i)} pairs of {nq} queries, survivors {surv} of {nq * n}, ties in {(t > 0).sum()} pairs, "
          f"bracket slack {int((g - lo).max())} / {int((up - g - t).max())}")
    assert cand.tolist() == cr.tolist()
    assert (lo <= g).all() and (g + t <= up).all(), f"{name}: outside the reference's bracket"
    # 3. top-k's lists
    if topk and n > 2:
        qs = np.unique(i)
        J, P, cnt = ctx.link_topk(qs + 1, 33, c["exclude"])
        qi = np.repeat(qs, cnt)
        r = np.concatenate([np.arange(m) for m in cnt])
        jj = np.concatenate([J[q, : cnt[q]] - 1 for q in range(len(qs))])
        g2, t2, _, p2 = _exactly(ctx, n, qi, jj, c["edges"], c["directed"], c["exclude"], name + " (top-k's pairs)")
        assert p2.tobytes() == np.concatenate([P[q, : cnt[q]] for q in range(len(qs))]).tobytes()
        assert ((g2 <= r) & (r <= g2 + t2)).all(), f"{name}: a top-k position outside greater .. greater + ties"


@pytest.mark.parametrize("shape", rr.RANK_SHAPES, ids=lambda s: "n%d-d%d-Qu%d-x%d-%s-%s" % (s[0], s[1], s[2], s[3], "dir" if s[4] else "und",
                                                                                          "excl" if s[5] else "all"))
def test_rank_shapes(ctx, shape):
    _check(ctx, rr.shape_case(*shape), "shape")


@pytest.mark.parametrize("shape", rr.RANK_SHAPES, ids=lambda s: "n%d-d%d-Qu%d-x%d-%s-%s" % (s[0], s[1], s[2], s[3], "dir" if s[4] else "und",
                                                                                          "excl" if s[5] else "all"))
def test_rank_shapes_with_several_tiles_per_workgroup(ctx, shape):
    """link_rank_kernel slices the candidate tiles as top-k does (nsl = min(ceil(2 cus / nQt), nTc, 512)): one tile per workgroup
    in every shape on 256 CUs.  Under the testing knob test_device_cus = 1 a workgroup walks up to half of them, its thresholds,
    the proven-pairs mask in the Gram staging and its row tables carried from tile to tile.  (The counts under knobs 1, 3 and 0
    are compared bit for bit in tests/test_gpu_link.py::test_link_queries_do_not_depend_on_the_cu_count.)"""
    ctx.set_option("test_device_cus", 1)
    try:
        _check(ctx, rr.shape_case(*shape), "shape, knob 1")
    finally:
        ctx.set_option("test_device_cus", 0)


_STRESS = rr.stress_cases()


@pytest.mark.parametrize("name", sorted(_STRESS))
def test_rank_cases(ctx, name):
    _check(ctx, _STRESS[name], name)


def test_rank_does_not_depend_on_the_other_pairs_or_their_order(ctx):
    """A pair's counts are a function of the inputs alone: asked alone, among 300 others (other rows of the tile, other
    thresholds of its own query) and in reversed order."""
    c = rr.shape_case(1000, 17, 129, 65, False, True, 31)
    _resident(ctx, c["X"], c["edges"])
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], None, False)
    i, j = c["i"][:301] + 1, c["j"][:301] + 1
    full = ctx.link_rank(i, j, True)
    rev = ctx.link_rank(i[::-1].copy(), j[::-1].copy(), True)
    for a, b in zip(full, rev):
        assert a.tobytes() == b[::-1].tobytes()
    for q in (0, 17, 300):
        one = ctx.link_rank(i[q:q + 1], j[q:q + 1], True)
        assert [int(x[0]) for x in one[:3]] == [int(x[q]) for x in full[:3]] and one[3][0] == full[3][q]
    assert ctx.get_stat("link_rank_queries") == 1


# ---- fitted models ----------------------------------------------------------------------------------------------------------------
def _held_out(g, seed):
    """5 % of the edge rows removed (pairs with both orientations or repeats among the rows are left alone: a held-out edge is not
    resident): the training graph and the removed pairs, 1-based."""
    e = np.asarray(g["edges"])
    rng = np.random.default_rng(seed)
    und = np.sort(e, axis=1)
    _, inv, counts = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    single = np.flatnonzero((counts[inv.ravel()] == 1) & (e[:, 0] != e[:, 1]))
    out = rng.choice(single, max(1, len(e) // 20), replace=False)
    keep = np.ones(len(e), bool)
    keep[out] = False
    return np.asfortranarray(e[keep]), np.asarray(g["eweights"])[keep], e[out]


@pytest.mark.parametrize("land", ["landmarks", "exact"])
@pytest.mark.parametrize("name", ["test115", "abcd2000"])
def test_rank_of_held_out_edges_under_a_fitted_model(test115, name, land):
    from cge.jl_amd import api, synth

    g = dict(test115) if name == "test115" else synth.abcd_like(2000, 20000, 12, 16, seed=52, directed=False)
    lm = -1 if land == "exact" else (20 if name == "test115" else 60)
    n = len(g["vweights"])
    train, tw, test = _held_out(g, 7)
    c = api.Context(0)
    try:
        c.set_inputs(train, tw, g["vweights"], g["comm"], g["embedding"])
        vec, _ = c.link_fit(g["clusters"], lm, forced=4, method="rss", directed=False, split=False, seed=17, auc_samples=2000)
        assert len(vec) == 7
        i, j = test[:, 0] - 1, test[:, 1] - 1
        g_, t_, cand, p = _exactly(c, n, i, j, np.asarray(train) - 1, False, True, f"{name} {land}")
        m = api.link_metrics(g_, t_, cand)
        print(f"  {name} {land}: {len(i)} held-out edges, alpha {c.link_model()['alpha']}, survivors "
              f"{c.get_stat('link_rank_survivors')} of {len(set(i.tolist())) * n}, {m}")
        assert m["auc"] > 0.5  # a sanity bound, not a measurement
        assert (cand > 0).all() and (g_ + t_ <= cand).all()
    finally:
        c.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_model_is_dropped_and_arguments_are_checked(ctx, test115):
    from cge.jl_amd import api

    g = test115
    n = len(g["vweights"])
    one = np.ones(n)

    def raises(msg, fn, *args):
        with pytest.raises(api.CGEError) as e:
            fn(*args)
        assert e.value.code == -7 and msg in str(e.value), str(e.value)

    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    ctx.link_set_model(2.0, 10.0, one)
    assert ctx.link_rank([1], [2])[2][0] > 0
    ctx.set_embedding(g["embedding"])
    raises("no link model", ctx.link_rank, [1], [2])
    ctx.link_set_model(2.0, 10.0, one)
    raises("P = 0", ctx.link_rank, [], [])
    raises("vertex 0", ctx.link_rank, [1, 0], [2, 3])
    raises(f"vertex {n + 1}", ctx.link_rank, [1], [n + 1])
    raises("not its own candidate", ctx.link_rank, [1, 5], [2, 5])
    with pytest.raises(ValueError):
        ctx.link_rank([1, 2], [3])
    assert ctx.link_rank([1], [2])[2][0] > 0  # the model survived them
    ctx.set_collectives(lambda user, buf, count, op: 0, 0, 2)  # (refused before the hook is ever called)
    try:
        raises("collectives", ctx.link_rank, [1], [2])
    finally:
        ctx.clear_collectives()
    assert ctx.link_rank([1], [2])[2][0] > 0


# ---- cge_links.py --rank ----------------------------------------------------------------------------------------------------------
def test_cge_links_rank_prints_link_ranks_values(tmp_path, capsys):
    from cge.jl_amd import api

    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    from cge_cli import julia_float

    gdir = os.path.join(ROOT, "tests", "golden", "test115")
    raw = api.read_table(f"{gdir}/test.edgelist", column_major=False)[0][:, :2].astype(np.int64)
    base, n = int(raw.min()), int(raw.max() - raw.min() + 1)
    rng = np.random.default_rng(3)
    i = rng.integers(0, n, 40)
    j = (i + 1 + rng.integers(0, n - 1, 40)) % n
    pf = tmp_path / "held_out.txt"
    pf.write_text("".join(f"{a + base} {b + base}\n" for a, b in zip(i, j)))
    argv = ["-g", f"{gdir}/test.edgelist", "-c", f"{gdir}/test1col.ecg", "-e", f"{gdir}/test_n2v.embedding", "-l", "20", "--seed", "5",
            "--samples-local", "2000", "--rank", str(pf)]
    for extra, exclude in (([], True), (["--keep-edges"], False)):
        assert cge_links.main(argv + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert lines[0].startswith("[") and len(lines) == 1 + 40 + 1
        g, t, cand, p = api.default_context().link_rank(i + 1, j + 1, exclude)  # the model main() fitted is still resident
        for q in range(40):
            assert lines[1 + q] == f"{i[q] + base} {j[q] + base} {julia_float(float(p[q]))} {g[q]} {t[q]} {cand[q]}"
        assert lines[-1] == cge_links.metrics_line(api.link_metrics(g, t, cand)) and lines[-1].startswith("# mrr=")
    assert cge_links.main(argv + ["--pairs", str(pf)]) == 1  # --rank excludes --pairs
