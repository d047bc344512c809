"""The link model on the device (`pytest -m gpu`): cge_link_set_model / cge_link_prob / cge_link_topk against the plain reference
of tests/link_ref.py on supplied models, and cge_link_fit against cge_score and against the local score it reports.

For every query of a top-k call the test asserts: the reported p are link_prob's values for those pairs, bit for bit; they agree
with the reference within its derived bound; the lists are sorted by (p descending, j ascending), hold admissible, distinct
candidates and the right count; and the smallest reference value among the returned candidates is at least (1 - 2 BOUND) times the
largest reference value among the admissible candidates left out.  Where tests/test_link_ref.py has shown the reference's order
to be beyond the reach of rounding (`exact`), the ids are compared one by one.

The slices of the candidate tiles follow the CU count: nsl = min(ceil(2 cus / nQt), nTc, 512).  On 256 CUs every shape below has
nsl == nTc, one tile per workgroup: no threshold ever moves before it is read, no list merges into an earlier one.  So the shapes
and the cases run a second time under the testing knob test_device_cus = 1 (nsl <= 2: four to eight tiles per workgroup at
n = 1000), and what that reaches is asserted, not hoped for: `descending_scores` must leave survivors below Q (n - 1) (its
thresholds provably reject whole tiles), `near_threshold` has entries that pass a moved threshold by 2e-4 of its squared radius.
link_merge_kernel keeps 8 list heads per lane; the merge tests run it on 66 slices (lanes 0 and 1 hold two heads) and on the cap
of 512 (every head, and slices that walk two tiles).  Scratch mutants (not committed) and what noticed them:
link_filter_thresholds' squared radius divided by 1 + 1e-3 -- near_threshold under knob 1 and in the test of the CU counts
(the last entry of both lists), no other case of either (random inputs put nothing that close to a threshold), and none of the
earlier tests at knob 0 (61 tests of top-k and rank); link_merge_kernel reading head 0 alone -- both merge tests and nothing
else."""
import contextlib
import ctypes as C
import functools
import math

import numpy as np
import pytest

import link_ref as lr

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def _knob(ctx, cus):
    """The context's launches sized for `cus` CUs (testing knob test_device_cus; 0: the device's own), and back."""
    if cus > _cus():
        pytest.skip("the device has %d CUs, the case asks for %d (test_device_cus only shrinks)" % (_cus(), cus))
    ctx.set_option("test_device_cus", cus)
    try:
        yield
    finally:
        ctx.set_option("test_device_cus", 0)


def _resident(ctx, X, edges0):
    n = len(X)
    e = np.asfortranarray(np.asarray(edges0, np.int64).reshape(-1, 2) + 1)
    ctx.set_graph(e, np.ones(len(e)), n)
    ctx.set_embedding(np.asfortranarray(X))


def _within_bound(got, ref):
    ref = np.asarray(ref, LD)
    err = np.abs(np.asarray(got, LD) - ref)
    ok = err <= lr.BOUND * ref
    worst = float((err / np.where(ref > 0, ref, 1)).max()) if len(ref) else 0.0
    return bool(ok.all()), worst


# ---- cge_link_prob ----------------------------------------------------------------------------------------------------------------
_PROB = {}


def _prob_input(d):
    if d not in _PROB:
        X = lr.points(300, d, 40 + d)
        X[200:250] = X[0:50]  # duplicated rows: distance 0
        hi, ai, aj = lr.diameter(X)
        rng = np.random.default_rng(d)
        _PROB[d] = (X, hi, ai, aj, np.exp(0.5 * rng.standard_normal(300)), np.exp(0.5 * rng.standard_normal(300)))
    return _PROB[d]


def _pairs(P, ai, aj, seed):
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, 300, P), rng.integers(0, 300, P)
    special = [(ai, aj), (aj, ai), (7, 7), (3, 203), (203, 3), (0, 299)]  # the diameter, i == j, a duplicated row, the corners
    for q, (a, b) in enumerate(special[:P]):
        i[q], j[q] = a, b
    return i, j


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("d", [1, 3, 8, 17])
def test_link_prob_against_the_reference(ctx, d, directed):
    X, hi, ai, aj, fo, fi = _prob_input(d)
    _resident(ctx, X, [(0, 1)])
    ctx.link_set_model(2.75, hi, fo, fi if directed else None, directed)
    for P in (1, 255, 256, 257, 5000):
        i, j = _pairs(P, ai, aj, P)
        got = ctx.link_prob(i + 1, j + 1)
        ref = lr.prob(X, hi, 2.75, fo, fi if directed else None, i, j)
        ok, worst = _within_bound(got, ref)
        print(f"  d={d} directed={directed} P={P}: worst relative error {worst:.3g} (bound {lr.BOUND:.3g})")
        assert ok
        assert got[0] == 0.0  # the pair attaining the diameter
        if P >= 6:
            assert got[2] == fo[7] * (fi if directed else fo)[7] and got[3] == fo[3] * (fi if directed else fo)[203]  # distance 0
        if not directed:
            assert np.array_equal(got, ctx.link_prob(j + 1, i + 1))  # symmetric, bit for bit


def test_link_prob_clamps_the_base_under_a_small_hi(ctx):
    X, hi, ai, aj, fo, fi = _prob_input(8)
    _resident(ctx, X, [(0, 1)])
    ctx.link_set_model(2.5, 0.5 * hi, fo, None, False)
    i, j = _pairs(5000, ai, aj, 9)
    got = ctx.link_prob(i + 1, j + 1)
    ref = lr.prob(X, 0.5 * hi, 2.5, fo, None, i, j)
    assert np.isfinite(got).all() and (got >= 0).all() and got[0] == 0.0
    assert ((got == 0) == (np.asarray(ref, np.float64) == 0)).all() and 0 < (got == 0).sum() < 5000
    assert _within_bound(got, ref)[0]


# ---- cge_link_topk ----------------------------------------------------------------------------------------------------------------
def _check_topk(ctx, c, name):
    X, k, n = c["X"], c["k"], len(c["X"])
    _resident(ctx, X, c["edges"])
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fi"], c["directed"])
    J, P, cnt = ctx.link_topk(c["queries"] + 1, k, c["exclude"])
    Jr, Pr, cntr, vals = lr.topk(X, c["hi"], c["alpha"], c["fo"], c["fi"], c["queries"], k, c["edges"], c["directed"], c["exclude"])
    assert J.shape == P.shape == (len(c["queries"]), k)
    assert cnt.tolist() == cntr.tolist()
    qi = np.repeat(c["queries"], cnt)
    jj = np.concatenate([J[q, : cnt[q]] - 1 for q in range(len(cnt))]) if cnt.sum() else np.zeros(0, np.int64)
    pp = np.concatenate([P[q, : cnt[q]] for q in range(len(cnt))]) if cnt.sum() else np.zeros(0)
    if len(jj):
        assert np.array_equal(pp, ctx.link_prob(qi + 1, jj + 1)), f"{name}: a reported p is not link_prob's"
        ok, worst = _within_bound(pp, lr.prob(X, c["hi"], c["alpha"], c["fo"], c["fi"], qi, jj))
        print(f"  {name}: {len(jj)} entries, worst relative error {worst:.3g} (bound {lr.BOUND:.3g}), "
              f"survivors {ctx.get_stat('link_topk_survivors')}")
        assert ok
    for q, (cand, pref) in enumerate(vals):
        m = int(cnt[q])
        j, p = J[q, :m] - 1, P[q, :m]
        assert (J[q, m:] == 0).all() and (P[q, m:] == 0.0).all()  # unused slots
        assert len(set(j.tolist())) == m and set(j.tolist()) <= set(cand.tolist())  # distinct and admissible
        assert all(p[t] > p[t + 1] or (p[t] == p[t + 1] and j[t] < j[t + 1]) for t in range(m - 1)), f"{name}: query {q} unsorted"
        inside = np.isin(cand, j)
        if m and (~inside).any():
            assert pref[inside].min() >= (1 - 2 * lr.BOUND) * pref[~inside].max(), f"{name}: query {q} misses a better candidate"
        if c.get("exact"):
            assert j.tolist() == Jr[q, :m].tolist(), f"{name}: query {q}"


@pytest.mark.parametrize("shape", lr.TOPK_SHAPES, ids=lambda s: "n%d-d%d-Q%d-k%d-%s-%s" % (s[0], s[1], s[2], s[3], "dir" if s[4] else "und",
                                                                                         "excl" if s[5] else "all"))
def test_topk_shapes(ctx, shape):
    _check_topk(ctx, lr.shape_case(*shape), "shape")


_STRESS = lr.stress_cases()


@pytest.mark.parametrize("name", sorted(_STRESS))
def test_topk_cases(ctx, name):
    _check_topk(ctx, _STRESS[name], name)


def SHAPE_ID(s):
    return "n%d-d%d-Q%d-k%d-%s-%s" % (s[0], s[1], s[2], s[3], "dir" if s[4] else "und", "excl" if s[5] else "all")


@pytest.mark.parametrize("shape", lr.TOPK_SHAPES, ids=SHAPE_ID)
def test_topk_shapes_with_several_tiles_per_workgroup(ctx, shape):
    with _knob(ctx, 1):
        _check_topk(ctx, lr.shape_case(*shape), "shape, knob 1")


@pytest.mark.parametrize("name", sorted(_STRESS))
def test_topk_cases_with_several_tiles_per_workgroup(ctx, name):
    c = _STRESS[name]
    with _knob(ctx, 1):
        _check_topk(ctx, c, name + ", knob 1")
        if name == "descending_scores":  # tests/test_link_ref.py: the k-th value after tile 0 is twice what a later tile holds
            Q, n = len(c["queries"]), len(c["X"])
            surv = ctx.get_stat("link_topk_survivors")
            print(f"  survivors {surv} of {Q * n}")
            assert Q * 128 <= surv < Q * (n - 1)  # the filter bites (and tile 0 is evaluated whole: the lists are short there)
            assert surv <= Q * (n - 3 * 128)  # the workgroup of tile 0 rejects its three later tiles whole


_CU_CASES = [lr.TOPK_SHAPES[8], lr.TOPK_SHAPES[9], lr.TOPK_SHAPES[10], "far_heavy_vertex", "common_offset", "near_threshold"]


@pytest.mark.parametrize("case", _CU_CASES, ids=lambda s: s if isinstance(s, str) else SHAPE_ID(s))
def test_link_queries_do_not_depend_on_the_cu_count(ctx, case):
    """include/cge_hip.h promises top-k's lists, rank's counts and a sample's edges as functions of the inputs alone: the same
    bits whatever the slices (knob 1: nsl <= 2, knob 3: nsl <= 6, the device's own)."""
    c = _STRESS[case] if isinstance(case, str) else lr.shape_case(*case)
    n, qs = len(c["X"]), c["queries"]
    _resident(ctx, c["X"], c["edges"])
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], c["fi"], c["directed"])
    ri = np.repeat(qs[:40], 3)
    rj = (ri * 7 + np.tile([1, 50, 333], len(qs[:40]))) % n
    rj = np.where(rj == ri, (rj + 1) % n, rj)
    got = {}
    for cus in (1, 3, 0):
        with _knob(ctx, cus):
            top = ctx.link_topk(qs + 1, c["k"], c["exclude"])
            surv = ctx.get_stat("link_topk_survivors")
            rank = ctx.link_rank(ri + 1, rj + 1, c["exclude"])
            smp = ctx.link_sample(5, 2, None, True)
            got[cus] = (top, rank, smp)
            print(f"  knob {cus}: top-k survivors {surv}, rank survivors {ctx.get_stat('link_rank_survivors')}, {smp[3]} sampled edges")
    for cus in (1, 3):
        for a, b in zip(got[cus][0], got[0][0]):  # J, P, cnt
            assert a.tobytes() == b.tobytes(), (case, cus, "top-k")
        for a, b in zip(got[cus][1], got[0][1]):  # greater, ties, cand, p
            assert a.tobytes() == b.tobytes(), (case, cus, "rank")
        assert got[cus][2][3] == got[0][2][3]
        for a, b in zip(got[cus][2][:3], got[0][2][:3]):  # i, j, p
            assert a.tobytes() == b.tobytes(), (case, cus, "sample")


# ---- link_merge_kernel with several heads per lane ----------------------------------------------------------------------------------
def _check_merge(ctx, n, nsl):
    """Q = 2, k = 64 on n candidates in nsl slices against a full sort of lr.prob's values (no O(n^2) diameter, no insertion
    loop): _check_topk's assertions."""
    c = lr.merge_case(n, 90)
    X, k, qs = c["X"], c["k"], c["queries"]
    assert (n + 127) // 128 >= nsl
    _resident(ctx, X, c["edges"])
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], None, False)
    J, P, cnt = ctx.link_topk(qs + 1, k, False)
    assert J.shape == P.shape == (2, k) and cnt.tolist() == [k, k]
    assert np.array_equal(P.ravel(), ctx.link_prob(np.repeat(qs, k) + 1, J.ravel())), "a reported p is not link_prob's"
    for q, i in enumerate(qs):
        cand = np.delete(np.arange(n), i)
        pref = lr.prob(X, c["hi"], c["alpha"], c["fo"], None, np.full(n - 1, i), cand)
        js, ps = lr.topk_by_sort(cand, pref, k)
        sl = (js // 128) % nsl
        assert (sl >= 64).sum() >= 8  # the reference's list has entries that a lane keeps under a head u >= 1
        j, p = J[q] - 1, P[q]
        ok, worst = _within_bound(p, pref[np.searchsorted(cand, j)])
        print(f"  n={n} query {i}: worst relative error {worst:.3g} (bound {lr.BOUND:.3g}); the reference's entries sit in "
              f"{len(set(sl.tolist()))} slices, {(sl >= 64).sum()} under heads >= 1, heads {sorted(set((sl // 64).tolist()))}")
        assert ok
        assert len(set(j.tolist())) == k and i not in j
        assert all(p[t] > p[t + 1] or (p[t] == p[t + 1] and j[t] < j[t + 1]) for t in range(k - 1)), f"query {q} unsorted"
        inside = np.isin(cand, j)
        assert pref[inside].min() >= (1 - 2 * lr.BOUND) * pref[~inside].max(), f"query {q} misses a better candidate"
        assert j.tolist() == js.tolist()  # (tests/test_link_ref.py: neighbours of the reference's list are > 2 BOUND apart)


def test_merge_with_two_heads_in_two_lanes(ctx):
    """n = 8321 under knob 33: nTc = 66 = nsl = ceil(2 x 33 / 1), so lanes 0 and 1 of link_merge_kernel hold two heads."""
    with _knob(ctx, 33):
        _check_merge(ctx, 8321, 66)


def test_merge_at_the_cap_of_512_slices(ctx):
    """n = 65700 on the device's own CU count: nTc = 514, nsl = min(2 cus, 514, 512) = 512 from 256 CUs on -- every lane holds 8
    heads, and the slices 0 and 1 walk two tiles."""
    if _cus() < 256:
        pytest.skip("the device has %d CUs: 2 cus slices stay below the cap of 512" % _cus())
    _check_merge(ctx, 65700, 512)


def test_topk_does_not_depend_on_the_query_batch(ctx):
    """A query's list is a function of the inputs alone: asked alone, or among 300 (another row tile, another row of it, other
    rows' thresholds beside its own)."""
    c = lr.shape_case(1000, 17, 300, 33, False, True, 31)
    _resident(ctx, c["X"], c["edges"])
    ctx.link_set_model(c["alpha"], c["hi"], c["fo"], None, False)
    J, P, cnt = ctx.link_topk(c["queries"] + 1, 33, True)
    for q in (0, 17, 299):
        j1, p1, c1 = ctx.link_topk(c["queries"][q:q + 1] + 1, 33, True)
        assert np.array_equal(j1[0], J[q]) and np.array_equal(p1[0], P[q]) and c1[0] == cnt[q]


# ---- fitted models ----------------------------------------------------------------------------------------------------------------
_GRAPHS = {}


def _graph(name, directed, test115):
    from cge.jl_amd import synth

    key = (name, directed)
    if key not in _GRAPHS:
        if name == "test115":
            g = dict(test115)
            g["land"] = 20
        elif name == "exact300":
            g = synth.abcd_like(300, 3000, 5, 8, seed=51, directed=directed)
            g["land"] = -1
        else:  # abcd2000 at -l 60 (a launch per fit iteration) and -l 300 (the fused persistent fit of a relabelled sweep)
            g = synth.abcd_like(2000, 20000, 12, 16, seed=52, directed=directed)
            g["land"] = int(name.split("-l")[1])
        _GRAPHS[key] = g
    return _GRAPHS[key]


def _fresh(g):
    from cge.jl_amd import api

    c = api.Context(0)
    c.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    return c


def _bits(tr):
    return tr["n_alpha"], np.asarray(tr["iters"]).tobytes(), np.asarray(tr["div"]).tobytes(), np.asarray(tr["auc"]).tobytes()


SEED, S = 17, 2000


@pytest.mark.parametrize("which", ["local", "global"])
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("name", ["test115", "abcd2000-l60", "abcd2000-l300", "exact300"])
def test_link_fit(test115, name, directed, which):
    from cge.jl_amd import api

    g = _graph(name, directed, test115)
    land, exact = g["land"], g["land"] == -1
    kw = dict(forced=4, method="rss", directed=directed, split=False, seed=SEED, auc_samples=S)
    a, b = _fresh(g), _fresh(g)
    try:
        # ---- the same results as cge_score on a fresh context: the capture changes nothing
        vec, tr = a.link_fit(g["clusters"], land, which=which, **kw)
        ref = b.score(g["clusters"], land, **kw)
        assert len(vec) == 7 and vec.tobytes() == ref.tobytes(), (vec, ref)
        assert _bits(tr) == _bits(b.last_trace)
        assert a.get_stat("fit_iterations") == b.get_stat("fit_iterations")
        # ---- the model's contents
        m = a.link_model()
        alpha = vec[4] if which == "local" else vec[0]
        ia = int(round(alpha / 0.25))
        assert m["alpha"] == alpha and m["directed"] == directed
        n = len(g["vweights"])
        X = np.ascontiguousarray(g["embedding"])
        if exact:
            assert len(m["T_out"]) == n and np.array_equal(m["f_out"], m["T_out"]) and np.array_equal(m["f_in"], m["T_in"])
            assert m["hi"] == lr.diameter(X)[0]  # the maximum of the exact-mode distances (dist()'s own arithmetic)
        else:
            lm = a.landmarks_fetch()
            lw, v2l = np.asarray(lm[5]), np.asarray(lm[6]) - 1
            vw = np.asarray(g["vweights"], np.float64)
            assert len(m["T_out"]) == len(lw)
            assert np.array_equal(m["f_out"], (m["T_out"][v2l] * vw) / lw[v2l])
            assert np.array_equal(m["f_in"], (m["T_in"][v2l] * vw) / lw[v2l])
            assert m["hi"] == a.last_diameter()[0]
        if not directed:
            assert np.array_equal(m["f_out"], m["f_in"]) and np.array_equal(m["T_out"], m["T_in"])
        # ---- the local score recomputed from link_prob's values on the sweep's own draws
        pos, ni, nj = (x[0] for x in api.draw_samples(a, SEED, S, directed))
        e = np.asarray(g["edges"])
        rows = pos
        if directed and exact:  # the overwriting second draw of :510; the weights stay the first draw's
            rows = a.draw_samples(SEED + 0x7777, S, True, stream_id=1000)[0]
        pi, pj = e[rows - 1, 0], e[rows - 1, 1]
        if not directed:
            pi, pj = np.minimum(pi, pj), np.maximum(pi, pj)
        w = np.asarray(g["eweights"], np.float64)[pos - 1]
        ppos, pneg = a.link_prob(pi, pj), a.link_prob(ni, nj)
        gap = np.abs(ppos - pneg)
        assert not (gap <= 1e-12 * np.maximum(ppos, pneg)).any(), "unsuitable input: a sample within reach of a last-bit flip"
        auc =1.0 - math.fsum(w[ppos > pneg]) / math.fsum(w)
        reported = vec[5] if which == "local" else tr["auc"][ia - 1]
        tol = (2 * S + 2) * 2.0 ** -53  # two sums of S terms, one rounding per addition, and the quotient and difference
        print(f"  {name} directed={directed} {which}: alpha {alpha}, auc {auc!r} reported {reported!r} (tolerance {tol:.3g})")
        if which == "global" and np.isnan(reported):
            # the local score's patience ran out before the best divergence's alpha (:213-223): the sweep tallied nothing there,
            # so the trace holds no figure to compare with (the local-best model of the same input is compared above)
            assert np.isnan(tr["auc"][ia - 1:tr["n_alpha"]]).all() and 0.0 <= auc <= 1.0
        else:
            assert abs(auc - reported) <= tol
        # ---- and the model answers queries
        j, p, cnt = a.link_topk(np.arange(1, 6), 5, True)
        assert (cnt == 5).all() and np.array_equal(p.ravel(), a.link_prob(np.repeat(np.arange(1, 6), 5), j.ravel()))
    finally:
        a.close()
        b.close()


def test_model_is_dropped_and_arguments_are_checked(ctx, test115):
    from cge.jl_amd import api

    g = test115
    n = len(g["vweights"])
    X = np.ascontiguousarray(g["embedding"])
    one = np.ones(n)

    def raises(msg, fn, *args):
        with pytest.raises(api.CGEError) as e:
            fn(*args)
        assert e.value.code == -7 and msg in str(e.value), str(e.value)

    def model():
        ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
        ctx.link_set_model(2.0, 10.0, one)

    # whatever replaces the resident inputs drops the model
    for drop in (lambda: ctx.set_embedding(g["embedding"]), lambda: ctx.set_embedding_view(X.astype(np.float32)),
                 lambda: ctx.set_graph(g["edges"], g["eweights"], n), lambda: ctx.set_graph_view(np.asarray(g["edges"]).T.copy(), n=n),
                 lambda: ctx.set_vertex_data(g["comm"], g["vweights"]), lambda: ctx.set_vertex_view(g["comm"], None)):
        model()
        assert ctx.link_prob([1], [2])[0] > 0
        drop()
        raises("no link model", ctx.link_prob, [1], [2])
        raises("no link model", ctx.link_topk, [1], 3)
        raises("no link model", ctx.link_model)
    # argument errors, each with its message
    model()
    raises("k = 0", ctx.link_topk, [1], 0)
    raises("k = 65", ctx.link_topk, [1], 65)
    raises("vertex 0", ctx.link_topk, [1, 0], 3)
    raises(f"vertex {n + 1}", ctx.link_topk, [n + 1], 3)
    raises("vertex 0", ctx.link_prob, [0], [1])
    raises(f"vertex {n + 1}", ctx.link_prob, [1], [n + 1])
    assert ctx.link_prob([1], [2])[0] > 0  # the model survived them
    bad = one.copy()
    bad[5] = -1.0
    nan = one.copy()
    nan[7] = np.nan
    for msg, args in (("n = ", (2.0, 10.0, one[:-1])), ("alpha", (0.0, 10.0, one)), ("alpha", (np.inf, 10.0, one)),
                      ("hi", (2.0, -1.0, one)), ("hi", (2.0, np.nan, one)), ("f_out[6]", (2.0, 10.0, bad)),
                      ("f_out[8]", (2.0, 10.0, nan)), ("f_in[6]", (2.0, 10.0, one, bad, True)), ("one factor", (2.0, 10.0, one, one * 2))):
        raises(msg, ctx.link_set_model, *args)
    assert ctx.link_prob([1], [2])[0] > 0  # a refused model leaves the resident one
    olen = C.c_int(7)
    raises("which = 3", lambda: ctx._check(ctx.L.cge_link_fit(ctx.h, C.byref(api.ScoreArgs()), C.c_int(3), api._p(one),
                                                               C.byref(olen), None)))
    raises("auc_samples", lambda: ctx.link_fit(g["clusters"], 20, auc_samples=0, which="local"))
    # no resident inputs at all
    c2 = api.Context(0)
    try:
        raises("must be resident", c2.link_set_model, 2.0, 10.0, one)
    finally:
        c2.close()


def test_link_fit_is_refused_under_collectives(ctx, test115):
    from cge.jl_amd import api

    g = test115
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    ctx.set_collectives(lambda user, buf, count, op: 0, 0, 2)  # (refused before the hook is ever called)
    try:
        with pytest.raises(api.CGEError) as e:
            ctx.link_fit(g["clusters"], 20, seed=3, auc_samples=500)
        assert e.value.code == -7 and "collectives" in str(e.value)
    finally:
        ctx.clear_collectives()


def test_directed_star_returns_six_elements_and_no_model(ctx):
    from cge.jl_amd import api

    n = 40
    edges = np.asfortranarray(np.stack([np.ones(n - 1, np.int64), np.arange(2, n + 1)], axis=1))
    comm = np.asfortranarray(((np.arange(n) % 2) + 1).reshape(-1, 1).astype(np.int64))
    emb = np.asfortranarray(lr.points(n, 4, 61))
    vw = np.ones(n)
    ctx.set_inputs(edges, np.ones(n - 1), vw, comm, emb)
    ctx.link_set_model(2.0, 10.0, vw)
    clusters = [np.flatnonzero(comm[:, 0] == q) + 1 for q in (1, 2)]
    vec, _ = ctx.link_fit(clusters, -1, directed=True, seed=5, auc_samples=200)
    assert len(vec) == 6
    with pytest.raises(api.CGEError) as e:
        ctx.link_prob([1], [2])
    assert "no link model" in str(e.value)
