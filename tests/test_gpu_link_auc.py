"""cge_link_auc on the device (`pytest -m gpu`): per resident edge the exact number of non-edges the model puts below it and
level with it, the exact local score and AUC.

The reference of every case is the definition evaluated on the device's own values: cge_link_prob of EVERY ordered pair, fetched,
and the counts taken in numpy on those bits (tests/link_auc_ref.py::counts) -- no tolerance anywhere.  out_p is cge_link_prob's
value of the row bit for bit, n_neg the count of the sampler's non-edges, the summary the long-double sums in the list's order."""
import os
import sys

import numpy as np
import pytest

import link_auc_ref as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _resident(ctx, c, weights=None):
    n = len(c["X"])
    e = np.asfortranarray(np.asarray(c["edges"], np.int64).reshape(-1, 2) + 1)
    ctx.set_graph(e, np.ones(len(e)) if weights is None else weights, n)
    ctx.set_embedding(np.asfortranarray(c["X"]))
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fi"], c["directed"])


def _device_table(ctx, n):
    """cge_link_prob of every ordered pair: (n, n)."""
    a, b = np.divmod(np.arange(n * n, dtype=np.int64), n)
    return ctx.link_prob(a + 1, b + 1).reshape(n, n)


def _check(ctx, c, name, weights=None, P=None):
    """One case against the definition on the device's values; returns (result, the three stats)."""
    _resident(ctx, c, weights)
    n, e = len(c["X"]), c["edges"]
    P = _device_table(ctx, n) if P is None else P
    less, ties, pe, nneg = ar.counts(P, e, c["directed"])
    r = ctx.link_auc(want_counts=True, want_p=True)
    stats = tuple(ctx.get_stat(k) for k in ("link_auc_survivors", "link_auc_proven", "link_auc_tiles"))
    pairs = n * (n - 1) if c["directed"] else n * (n - 1) // 2
    print(f"  {name}: n {n} m {len(e)} neg {nneg}, survivors {stats[0]} proven {stats[1]} of {pairs} pairs, tiles {stats[2]}, "
          f"ties in {(ties > 0).sum()} rows, local_exact {r['local_exact']}")
    assert r["p"].tobytes() == pe.tobytes() == ctx.link_prob(e[:, 0] + 1, e[:, 1] + 1).tobytes(), f"{name}: out_p is not link_prob's"
    assert r["n_pos"] == len(e) and r["n_neg"] == nneg == ar.n_neg_from_keys(n, e, c["directed"])
    bad = np.flatnonzero((r["less"] != less) | (r["ties"] != ties))
    assert len(bad) == 0, (f"{name}: {len(bad)} of {len(e)} rows differ from the definition; first: row {bad[0]} = {e[bad[0]]} got "
                           f"{(r['less'][bad[0]], r['ties'][bad[0]])} expected {(less[bad[0]], ties[bad[0]])}")
    assert (r["W"], r["L"], r["Tq"]) == ar.summary(less, ties, weights)
    if nneg > 0:
        den = LD(r["W"]) * LD(nneg)
        assert r["local_exact"] == float(LD(1) - LD(r["L"]) / den) and r["auc"] == float((LD(r["L"]) + LD(r["Tq"]) / LD(2)) / den)
    else:
        assert np.isnan(r["local_exact"]) and np.isnan(r["auc"]) and not less.any() and not ties.any()
    assert stats[0] + stats[1] == pairs and stats[2] == len(ar.tile_positions(n, c["directed"]))  # every pair is settled once
    short = ctx.link_auc()  # no arrays asked for: the same sums
    assert repr({k: short[k] for k in short}) == repr({k: r[k] for k in short})  # (repr: a NaN equals itself)
    return r, stats


_IDS = lambda s: "n%d-d%d-m%d-%s" % (s[0], s[1], s[2], "dir" if s[3] else "und")  # noqa: E731


@pytest.mark.parametrize("shape", ar.AUC_SHAPES, ids=_IDS)
def test_auc_shapes(ctx, shape):
    _check(ctx, ar.shape_case(*shape), "shape")


def test_auc_with_edge_weights(ctx):
    """W, L and Tq take the resident weights in the list's order."""
    c = ar.shape_case(300, 32, 900, False, 21)
    w = np.random.default_rng(21).random(len(c["edges"])) + 0.25
    r, _ = _check(ctx, c, "weights", weights=w)
    assert r["W"] != float(len(w))


def test_both_sides_of_the_filter_act(ctx):
    """"link_auc_proven" adds the two sides up, so each is shown where the other cannot act.  A self loop on the heaviest vertex
    is the largest threshold by far (f^2 at distance 0, above every pair's value): nothing can be proven above it, so what is
    proven is proven BELOW the smallest.  A positive of probability 0 (a zero factor) makes the smallest threshold 0: nothing is
    below it, so what is proven is proven ABOVE the largest."""
    c = ar.shape_case(1000, 32, 4000, False, 22)
    v = int(np.argmax(c["fo"]))
    c["edges"][3] = (v, v)
    _, st = _check(ctx, c, "below")
    assert st[1] > 0 and st[0] > 0
    c = ar.shape_case(1000, 32, 4000, False, 23)
    c["edges"] = c["edges"][np.arange(len(c["edges"])) != 3]  # (no self loop)
    z = int(c["edges"][10, 0])
    c["fo"][z] = 0.0
    _, st = _check(ctx, c, "above")
    assert st[1] > 0 and st[0] > 0


_STRESS = ar.stress_cases()


@pytest.mark.parametrize("name", sorted(_STRESS))
def test_auc_cases(ctx, name):
    r, _ = _check(ctx, _STRESS[name], name)
    if name in ("ties_between_positives_and_negatives", "zero_factor", "small_hi_dir0", "small_hi_dir1"):
        assert r["Tq"] > 0  # exact ties between positives and negatives really occur


def test_power_forms(ctx, test115):
    """A fitted exact-mode model takes the power in the stored-logarithm form under the option pow_exp2 and the library pow
    without it: both kernels, against cge_link_prob's values of the same form."""
    g = test115
    n = len(g["vweights"])
    for opt in (1, 0):
        ctx.set_option("pow_exp2", opt)
        try:
            ctx.set_inputs(g["edges"], np.ones(len(g["edges"])), g["vweights"], g["comm"], g["embedding"])
            vec, _ = ctx.link_fit(g["clusters"], -1, forced=4, method="rss", directed=False, split=False, seed=17, auc_samples=500)
            assert len(vec) == 7
            m = ctx.link_model()
            c = dict(X=np.asarray(g["embedding"], np.float64), edges=np.asarray(g["edges"], np.int64) - 1, directed=False)
            P = _device_table(ctx, n)
            less, ties, pe, nneg = ar.counts(P, c["edges"], False)
            r = ctx.link_auc(want_counts=True, want_p=True)
            assert r["p"].tobytes() == pe.tobytes() and r["n_neg"] == nneg
            assert r["less"].tolist() == less.tolist() and r["ties"].tolist() == ties.tolist()
            print(f"  pow_exp2 {opt}: alpha {m['alpha']} local_exact {r['local_exact']} sampled {vec[5]}")
        finally:
            ctx.set_option("pow_exp2", 1)


@pytest.mark.parametrize("cus", [2, 8])
def test_auc_does_not_depend_on_the_cu_count(ctx, cus):
    """Two workgroups per CU walk the tiles by stride: under the testing knob test_device_cus a workgroup walks several (n = 1000
    undirected: 36 tiles on 4 or 16 workgroups), its row tables and masks carried from tile to tile.  Identical arrays."""
    cases = [ar.shape_case(*ar.AUC_SHAPES[7]), ar.shape_case(*ar.AUC_SHAPES[8]), ar.shape_case(*ar.AUC_SHAPES[5]),
             _STRESS["ties_between_positives_and_negatives"], _STRESS["zero_factor"]]
    for k, c in enumerate(cases):
        _resident(ctx, c)
        full = ctx.link_auc(want_counts=True, want_p=True)
        ctx.set_option("test_device_cus", cus)
        try:
            r, _ = _check(ctx, c, f"case {k}, knob {cus}")
        finally:
            ctx.set_option("test_device_cus", 0)
        for key in ("less", "ties", "p"):
            assert r[key].tobytes() == full[key].tobytes()
        assert (r["n_neg"], r["W"], r["L"], r["Tq"]) == (full["n_neg"], full["W"], full["L"], full["Tq"])


@pytest.mark.parametrize("directed", [False, True])
def test_parts_add_up_exactly(ctx, directed):
    """n = 300: 6 tiles (directed: 9).  The per-part arrays of 2, 7 and 64 parts sum to the arrays of one call; n_neg is the whole
    graph's in every part; a part without tiles returns zeros."""
    from cge.jl_amd import api

    c = ar.shape_case(300, 5, 600, directed, 11)
    _resident(ctx, c)
    whole = ctx.link_auc(want_counts=True)
    tiles = sorted(ar.tile_positions(300, directed).values())
    for nparts in (2, 7, 64):
        less, ties, seen = np.zeros_like(whole["less"]), np.zeros_like(whole["ties"]), 0
        for part in range(nparts):
            r = ctx.link_auc(part, nparts, want_counts=True)
            mine = sum(1 for t in tiles if t % nparts == part)
            assert ctx.get_stat("link_auc_tiles") == mine and r["n_neg"] == whole["n_neg"] and r["W"] == whole["W"]
            if mine == 0:
                assert not r["less"].any() and not r["ties"].any() and r["L"] == 0.0 and r["Tq"] == 0.0
            less += r["less"]
            ties += r["ties"]
            seen += mine
        assert seen == len(tiles)
        assert less.tobytes() == whole["less"].tobytes() and ties.tobytes() == whole["ties"].tobytes()
        s = api.link_auc_from_counts(less, ties, None, whole["n_neg"])
        assert (s["local_exact"], s["auc"], s["L"], s["Tq"]) == (whole["local_exact"], whole["auc"], whole["L"], whole["Tq"])


# ---- fitted models ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,land,seed,S", ar.FITTED, ids=lambda v: str(v))
def test_the_sampled_score_is_within_five_sigmas_of_the_exact_one(test115, name, land, seed, S):
    """Element 6 of the vector is the mean of S independent Bernoulli(q) draws, q = local_exact of the model of its alpha (unit
    weights): |element 6 - q| <= 5 sqrt(q (1 - q) / S).  The seeds are fixed; tests/test_link_auc_ref.py holds their draws to the
    same condition on the CPU."""
    from cge.jl_amd import api, synth

    g = dict(test115) if name == "test115" else synth.abcd_like(2000, 20000, 12, 16, seed=52, directed=False)
    c = api.Context(0)
    try:
        c.set_inputs(g["edges"], np.ones(len(g["edges"])), g["vweights"], g["comm"], g["embedding"])
        vec, _ = c.link_fit(g["clusters"], land, forced=4, method="rss", directed=False, split=False, seed=seed, auc_samples=S,
                            which="local")
        assert len(vec) == 7
        r = c.link_auc()
        q = r["local_exact"]
        sd = np.sqrt(q * (1.0 - q) / S)
        print(f"  {name} land {land}: sampled {vec[5]} exact {q} ({(vec[5] - q) / sd:+.2f} sd), auc {r['auc']}, neg {r['n_neg']}, "
              f"survivors {c.get_stat('link_auc_survivors')} proven {c.get_stat('link_auc_proven')}")
        assert r["n_pos"] == len(g["edges"]) and 0.0 < q < 0.5
        assert ar.within_sigmas(vec[5], q, S), (vec[5], q, sd)
    finally:
        c.close()


def test_api_link_auc_on_tensors(test115):
    from cge.jl_amd import api

    g = test115
    c = api.Context(0)
    try:
        ei = (np.asarray(g["edges"]).T - 1).astype(np.int64)
        vec, r = api.link_auc(ei, np.ascontiguousarray(g["embedding"]), np.asarray(g["comm"]).ravel() - 1, 20, seed=17, auc_samples=2000,
                              want_counts=True, base=0, ctx=c)
        assert len(vec) == 7 and r["n_pos"] == ei.shape[1] and len(r["less"]) == ei.shape[1]
        again = c.link_auc(want_counts=True)
        assert again["less"].tobytes() == r["less"].tobytes() and again["local_exact"] == r["local_exact"]
    finally:
        c.close()


# ---- consistency with cge_link_rank -------------------------------------------------------------------------------------------------
def test_consistent_with_link_rank(ctx):
    """For rows e = (i, j): link_rank(i, j, exclude_edges) ranks j among the non-neighbours c of i on the same values, so the
    negatives that contain i as the source split as cand - greater - ties below, ties level.  Directed: exactly the negatives
    (i, c).  Checked against the device table by brute force for the same rows."""
    c = ar.shape_case(300, 5, 299, True, 5)
    _resident(ctx, c)
    n, e = 300, c["edges"]
    P = _device_table(ctx, n)
    rows = [r for r in range(len(e)) if e[r, 0] != e[r, 1]][:8]
    g, t, cand, p = ctx.link_rank(e[rows, 0] + 1, e[rows, 1] + 1, True)
    neg = ar.negatives_mask(n, e, True)
    for k, r in enumerate(rows):
        i = int(e[r, 0])
        v = P[i][neg[i]]
        assert cand[k] == len(v) and g[k] == (v > p[k]).sum() and t[k] == (v == p[k]).sum()
        assert p[k] == P[i, e[r, 1]]


# ---- errors and lifetime ------------------------------------------------------------------------------------------------------------
def test_errors_and_lifetime(ctx, test115):
    import ctypes as C

    from cge.jl_amd import api

    g = test115
    n = len(g["vweights"])
    one = np.ones(n)

    def raises(msg, fn, *args):
        with pytest.raises(api.CGEError) as e:
            fn(*args)
        assert e.value.code == -7 and msg in str(e.value), str(e.value)

    def raw(part, nparts, nneg=True, summ=True):
        nn, sm = C.c_int64(), np.zeros(3)
        return ctx.L.cge_link_auc(ctx.h, C.c_int(part), C.c_int(nparts), None, None, None, C.byref(nn) if nneg else None,
                                  sm.ctypes.data if summ else None)

    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    ctx.link_set_model(2.0, 10.0, one)
    ok = ctx.link_auc()
    assert ok["n_neg"] > 0 and 0.0 < ok["auc"] < 1.0
    ctx.set_embedding(g["embedding"])
    raises("no link model", ctx.link_auc)
    ctx.link_set_model(2.0, 10.0, one)
    for part, nparts in ((0, 0), (-1, 2), (2, 2)):
        assert raw(part, nparts) == -7 and "part" in ctx.L.cge_last_error(ctx.h).decode()
        assert ctx.link_auc() == ok  # the context is usable after each error, the model survived
    assert raw(0, 1, nneg=False) == -7 and raw(0, 1, summ=False) == -7
    assert ctx.link_auc() == ok
    ctx.set_collectives(lambda user, buf, count, op: 0, 0, 2)  # (refused before the hook is ever called)
    try:
        raises("collectives", ctx.link_auc)
    finally:
        ctx.clear_collectives()
    assert ctx.link_auc() == ok
    with pytest.raises(ValueError):
        ctx.link_auc(3, 2)


# ---- cge_links.py --auc -------------------------------------------------------------------------------------------------------------
def test_cge_links_auc_prints_link_aucs_values(capsys):
    from cge.jl_amd import api

    sys.path.insert(0, ROOT)
    try:
        import cge_links
    finally:
        sys.path.pop(0)
    gdir = os.path.join(ROOT, "tests", "golden", "test115")
    argv = ["-g", f"{gdir}/test.edgelist", "-c", f"{gdir}/test1col.ecg", "-e", f"{gdir}/test_n2v.embedding", "-l", "20", "--seed", "5",
            "--samples-local", "2000", "--auc"]
    for extra in ([], ["--which", "global"]):
        assert cge_links.main(argv + extra) == 0
        lines = capsys.readouterr().out.strip().split("\n")
        assert lines[0].startswith("[") and len(lines) == 2
        c = api.default_context()  # the model main() fitted is still resident
        assert lines[1] == cge_links.auc_line(c.link_auc(), c.get_stat("link_auc_survivors")) and lines[1].startswith("# local_exact=")
    assert cge_links.main(argv + ["--sample", "x.txt"]) == 1  # --auc excludes --sample
