"""The persistent fits on the geometries of chips with fewer CUs, run on the chip at hand (run with -m gpu on an MI355X).

flow_geometry (kernels_fitp.hip) gives a workgroup TWO quarter blocks to reduce (NSB = 2) only where 4 Nt > G, which 256 CUs
never reach: fit_flow_kernel<1, NW, false, 2> and fit_flow_dir_kernel<NW, 2> run on a 32-CU partition of the same chip and in no
other test.  The testing knob test_device_cus (include/cge_hip_testing.h) tells the context a smaller CU count, and every launch
shape follows.  The rows (knob, N -> G, NW, NSB), asserted of the library's own geometry hook before anything runs:

  2    1, 7, 64     2, 4, 2   one tile, both workgroups hold two quarter blocks
  8    130, 256     8, 4, 2   ragged last tile; Nt = 4 with every workgroup at two quarter blocks
  32   513          32, 4, 2  Nt = 9: four workgroups hold a second quarter block, 28 do not
  32   960          32, 4, 2  Nt = 15, the last N on 4 waves
  32   961, 1024    32, 8, 2  8 waves with two quarter blocks; 1024 = a full last tile
  32   1025         declined  form 3 is CGE_E_ARG, form 0 runs form 1
  64   1409         64, 8, 2  the first N on 8 waves at 64 CUs

A row is skipped, with the reason, on a device with fewer CUs than its knob (the knob only shrinks).  The checks are those of
tests/test_gpu_fit.py, by its own helpers, against tests/fit_ref.py: V1 exact inputs, V2 one step within fr.step_bound with NaN
below the diagonal tiles, V3 K steps with iters == K within A_K times the bound (chains: fit_ref.SMALL_CHIP_*_CHAINS, pinned on
the CPU by tests/test_fit_ref.py), a second run, a start skew, the give-up path.  No tolerance of its own.

Bits against the same N at knob 0 (the NSB = 1 instance) ARE asserted.  The reducers (fit_flow_body.inc, fit_flow_dir_body.inc)
add a row's partial vectors as ((p[qg] + p[qg + 16]) + p[qg + 32]) + p[qg + 48] per thread and then qg = 0 .. 15 in order: the
order is a function of Nt alone.  G and NSB decide which workgroup reduces a quarter block, NW which wave owns a tile; neither
enters a sum.

Above the kernels: an exact-mode sweep (n = 700 undirected, 640 directed) and a landmark-mode score (600 landmarks, where NSB = 2
is not the fused geometry) under knob 32, and cge_score_batch of 5 members at 256 landmarks under knob 32 (G = 16 = cus / 2: two
members per launch group).

Measured on an MI355X (`-s` prints the figures), largest device error as a fraction of its tolerance, undirected / directed:
  knob 2: V2 0.084 / 0.091, V3 0.097 / 0.144;  knob 8: V2 0.039 / 0.024, V3 0.025 / 0.013;
  knob 32: V2 0.0085 / 0.0053, V3 0.0082 / 0.0036;  knob 64: V2 0.0043 / 0.0028, V3 0.0032 / 0.0014.
  A_K: 2.0 .. 3.92 undirected (K = 2 .. 45), 2.0 .. 2.41 directed (K = 2 .. 13).  The landmark-mode score of 600 landmarks had
  the bits of knob 0; the batches ran 85 / 88 launches for 127 / 133 member-alphas.
Scratch mutant (not committed): the reducers of NSB = 2 adding the second quarter block's sums twice (S += red[..][1][u] again
for i == 1, in both bodies) passes tests/test_gpu_fit.py at knob 0 (101 tests: the instances never run there) and fails V1, V2
and V3 of every row from N = 64 on, undirected and directed (at N = 1 and 7 the second quarter blocks hold no row of the matrix).
"""
import contextlib

import numpy as np
import pytest

import fit_ref as fr
import test_gpu_fit as tf

pytestmark = pytest.mark.gpu

LD = fr.LD
E_ARG = -7
ROWS = [(2, 1, (2, 4, 2)), (2, 7, (2, 4, 2)), (2, 64, (2, 4, 2)), (8, 130, (8, 4, 2)), (8, 256, (8, 4, 2)), (32, 513, (32, 4, 2)),
        (32, 960, (32, 4, 2)), (32, 961, (32, 8, 2)), (32, 1024, (32, 8, 2)), (64, 1409, (64, 8, 2))]
DECLINED = (32, 1025)
ROW_IDS = ["cus%d-N%d" % (c, n) for c, n, _ in ROWS]
FORMS = (0, 1, 3)  # what a sweep picks, the comparator, the persistent fit
TABLES = (fr.SMALL_CHIP_UNDIRECTED_CHAINS, fr.SMALL_CHIP_DIRECTED_CHAINS)
BOTH = pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
EACH_ROW = pytest.mark.parametrize("cus,N,geo", ROWS, ids=ROW_IDS)


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _knob(ctx, cus):
    """The context sized for `cus` CUs; back to the device's own afterwards, whatever happens."""
    if cus > tf._cus():
        pytest.skip("the device has %d CUs, the row asks for %d (test_device_cus only shrinks)" % (tf._cus(), cus))
    ctx.set_option("test_device_cus", cus)
    try:
        yield
    finally:
        ctx.set_option("test_device_cus", 0)


_cache = {}


def _cases(ctx, N, directed):
    if N in fr.UNDIRECTED_CHAINS:
        return tf._cases(ctx, N, directed)
    if (N, directed) not in _cache:  # (form 1 makes the power matrix: no launch shape in it)
        _cache[N, directed] = fr.chain_cases(N, directed, lambda pr, alpha: tf._device_gd(ctx, pr, directed), TABLES)
    return _cache[N, directed]


def test_the_rows_land_on_the_instances_named():
    from cge.jl_amd import api

    for cus, N, geo in ROWS:
        assert api.fit_dir_geometry_test(N, cus) == geo, (cus, N)
        g = tf._geometry(N, cus)
        assert g == (geo[0], geo[1], False) and 3 in tf._forms(N, False, cus=cus) and 4 not in tf._forms(N, False, cus=cus)
        assert tf._cus() < 4 * ((N + 63) // 64) or api.fit_dir_geometry_test(N, tf._cus())[2] == 1  # knob 0 is the other instance
    assert api.fit_dir_geometry_test(DECLINED[1], DECLINED[0]) is None and tf._geometry(DECLINED[1], DECLINED[0]) is None
    assert api.fit_dir_geometry_test(1408, 64) == (64, 4, 2)  # (1409 is the first on 8 waves)


def test_the_knob_only_shrinks(ctx):
    from cge.jl_amd import api

    for bad in (tf._cus() + 1, -1):
        with pytest.raises(api.CGEError) as e:
            ctx.set_option("test_device_cus", bad)
        assert e.value.code == E_ARG
    try:
        ctx.set_option("test_device_cus", tf._cus())  # the device's own count: allowed, and the same shapes
        pr = fr.random_undirected(130, 1.0, 1)
        a = tf._run(ctx, pr, False, 3, 1e-3)
    finally:
        ctx.set_option("test_device_cus", 0)
    assert tf._same(a, tf._run(ctx, pr, False, 3, 1e-3))


# ---- V1 --------------------------------------------------------------------------------------------------------------
@BOTH
@EACH_ROW
def test_exact_inputs_give_the_fp64_step_bit_for_bit(ctx, cus, N, geo, directed):
    pr, T1, f0 = fr.exact_problem(N, 40 + N, directed)
    eps = 0.5 if directed else 0.25
    with _knob(ctx, cus):
        for form in FORMS:
            out = tf._run(ctx, pr, directed, form, 2.0 * f0, eps=eps, cus=cus)
            assert out["iters"] == 1 and out["status"] == 0, (N, form, out["iters"], out["status"])
            if directed:
                assert np.array_equal(out["T"], T1[0]) and np.array_equal(out["Tb"], T1[1]), (N, form)
                if N >= 8:  # zero-degree rows come back as they started
                    assert np.array_equal(out["T"][[1, 3]], pr["T0"][[1, 3]]) and np.array_equal(out["Tb"][[2, 5]], pr["T0b"][[2, 5]])
            else:
                bad = np.flatnonzero(out["T"] != T1)
                assert bad.size == 0, (N, form, bad[:8], out["T"][bad[:8]], T1[bad[:8]])


# ---- V2 --------------------------------------------------------------------------------------------------------------
@EACH_ROW
def test_one_step_undirected_within_the_a_priori_bound(ctx, cus, N, geo):
    alpha = (1.0, 4.0, 10.0, 0.25)[N % 4]
    pr = fr.random_undirected(N, alpha, 300 + N)
    pr["T0"] = np.exp(0.3 * np.random.default_rng(N).normal(size=N))
    GD = tf._device_gd(ctx, pr, False)
    ref = fr.fit_undirected(GD, pr["T0"], pr["w"], 0.25, steps=1)
    tol = fr.step_bound(0.25, pr["T0"], pr["w"], ref["S"][0], ref["T"][1], N)
    delta = 2.0 * float(ref["f"][0])
    dirty = dict(pr, D=tf._nan_below_the_diagonal_tiles(pr["D"]))
    base = tf._run(ctx, dirty, False, 3, delta)  # knob 0
    with _knob(ctx, cus):
        for form in FORMS:
            out = tf._run(ctx, dirty, False, form, delta, cus=cus)
            assert out["iters"] == 1 and out["status"] == 0, (N, form)
            err = np.abs(LD(out["T"]) - ref["T"][1])
            assert np.all(err <= tol), (N, form, int(np.argmax(err / tol)), float(np.max(err / tol)))
            tf._note("V2 undirected, knob %d" % cus, np.max(err / tol))
            assert tf._same(out, tf._run(ctx, pr, False, form, delta, cus=cus)), (N, form)  # below the diagonal tiles: never read
            if form == 3:
                assert tf._same(out, base), (N, "knob 0")


@EACH_ROW
def test_one_step_directed_within_the_a_priori_bound(ctx, cus, N, geo):
    alpha = (1.0, 4.0, 10.0, 0.25)[N % 4]
    pr = fr.random_directed(N, alpha, 400 + N)
    rng = np.random.default_rng(N)
    pr["T0"], pr["T0b"] = np.exp(0.3 * rng.normal(size=N)), np.exp(0.3 * rng.normal(size=N))  # (zero-degree rows too: kept)
    GD = tf._device_gd(ctx, pr, True)
    ref = fr.fit_directed(GD, pr["T0"], pr["T0b"], pr["w"], pr["w2"], 0.9, steps=1)
    delta = 2.0 * float(ref["f"][0])
    base = tf._run(ctx, pr, True, 3, delta)  # knob 0
    with _knob(ctx, cus):
        for form in FORMS:
            out = tf._run(ctx, pr, True, form, delta, cus=cus)
            assert out["iters"] == 1 and out["status"] == 0, (N, form)
            for got, k, start, deg in ((out["T"], 0, pr["T0"], pr["w"]), (out["Tb"], 1, pr["T0b"], pr["w2"])):
                z = deg == 0
                assert np.array_equal(got[z], start[z]), (N, form, k)
                tol = fr.step_bound(0.9, start, deg, ref["S"][0][k], ref["T"][1][k], N)
                err = np.abs(LD(got) - ref["T"][1][k])
                if np.any(~z):
                    assert np.all(err[~z] <= tol[~z]), (N, form, k, float(np.max(err[~z] / tol[~z])))
                    tf._note("V2 directed, knob %d" % cus, np.max(err[~z] / tol[~z]))
            if form == 3:
                assert tf._same(out, base), (N, "knob 0")


# ---- V3, and the bits of knob 0 -------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("cus,N,geo", ROWS[1:], ids=ROW_IDS[1:])
def test_k_steps_to_a_chosen_end(ctx, cus, N, geo, directed):
    cases = _cases(ctx, N, directed)
    print(f"  N = {N}: K, A_K =", [(c["K"], round(c["A"], 2)) for c in cases])
    assert any(c["start"] == "prev" for c in cases) and any(c["K"] >= 3 for c in cases)
    base = [tf._run(ctx, c["problem"], directed, 3, c["delta"]) for c in cases]  # knob 0: NSB = 1 on a device of 4 Nt CUs or more
    with _knob(ctx, cus):
        for c, b in zip(cases, base):
            outs = tf._check_case(ctx, c, N, directed, FORMS, cus=cus, tag=", knob %d" % cus)
            assert tf._same(outs[3], outs[0]) if N >= 128 else tf._same(outs[1], outs[0])
            assert tf._same(outs[3], b), (N, directed, c["K"], "knob 0")


# ---- repeat, start skew -------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("cus,N,geo", ROWS[1:], ids=ROW_IDS[1:])
def test_a_second_run_and_a_start_skew_give_the_same_bits(ctx, cus, N, geo, directed):
    c = _cases(ctx, N, directed)[0]
    with _knob(ctx, cus):
        first = tf._run(ctx, c["problem"], directed, 3, c["delta"], cus=cus)
        assert first["iters"] == c["K"] and first["status"] == 0
        assert tf._same(first, tf._run(ctx, c["problem"], directed, 3, c["delta"], cus=cus)), (N, directed)
        try:
            ctx.set_option("fit_persistent_test_delay", 20)
            assert tf._same(first, tf._run(ctx, c["problem"], directed, 3, c["delta"], cus=cus)), (N, directed, "delay")
        finally:
            ctx.set_option("fit_persistent_test_delay", 0)


# ---- the give-up path ------------------------------------------------------------------------------------------------------------
def _problem(ctx, N, directed):
    """(problem, delta, eps, iterations): the second case of N's chain (a start that is not the sweep's); N = 1 has no chain and
    takes V1's exact problem, which ends after one iteration."""
    if N == 1:
        pr, _, f0 = fr.exact_problem(N, 40 + N, directed)
        return pr, 2.0 * f0, 0.5 if directed else 0.25, 1
    c = _cases(ctx, N, directed)[1]
    return c["problem"], c["delta"], None, c["K"]


@EACH_ROW
def test_an_abandoned_launch_writes_nothing(ctx, cus, N, geo):
    (und, du, eu, Ku), (drc, dd, ed, Kd) = _problem(ctx, N, False), _problem(ctx, N, True)
    with _knob(ctx, cus):
        want_u, want_d = tf._run(ctx, und, False, 1, du, eps=eu, cus=cus), tf._run(ctx, drc, True, 1, dd, eps=ed, cus=cus)
        assert (want_u["iters"], want_d["iters"]) == (Ku, Kd)
        try:
            ctx.set_option("fit_persistent_test_timeout", 1)
            out = tf._run(ctx, und, False, 3, du, eps=eu, cus=cus)
            assert out["status"] == 1 and np.all(np.isnan(out["T"])), (out["status"], out["T"][:4])
            out = tf._run(ctx, drc, True, 3, dd, eps=ed, cus=cus)  # Tin / Tout are updated on success only: the start comes back
            assert out["status"] == 1 and np.array_equal(out["T"], drc["T0"]) and np.array_equal(out["Tb"], drc["T0b"])
            ran, (out,) = ctx.fit_test(und, form=0, eps=eu, delta=du)  # the sweep's fallback: one launch per iteration
            assert ran == 1 and tf._same(out, want_u)
            ran, (out,) = ctx.fit_test(drc, directed=True, form=0, eps=ed, delta=dd)
            assert ran == 1 and tf._same(out, want_d)
        finally:
            ctx.set_option("fit_persistent_test_timeout", 0)
        back = tf._run(ctx, und, False, 3, du, eps=eu, cus=cus)  # and back
        assert back["status"] == 0 and back["iters"] == Ku


# ---- the declined row ------------------------------------------------------------------------------------------------------------
def test_the_declined_row(ctx):
    from cge.jl_amd import api

    cus, N = DECLINED
    und, drc = fr.random_undirected(N, 1.0, 2), fr.random_directed(N, 1.0, 2)
    with _knob(ctx, cus):
        for pr, directed in ((und, False), (drc, True)):
            with pytest.raises(api.CGEError) as e:
                ctx.fit_test(pr, directed=directed, form=3)
            assert e.value.code == E_ARG and "declines N = %d on %d CUs" % (N, cus) in str(e.value), str(e.value)
            auto = tf._run(ctx, pr, directed, 0, 1e300, cus=cus)  # (asserts that form 1 ran; one step, as test_gpu_fit.py's refusals)
            assert auto["status"] == 0 and auto["iters"] == 1 and tf._same(auto, tf._run(ctx, pr, directed, 1, 1e300, cus=cus))
    if tf._geometry(N):  # knob 0 again: the persistent form is back (asserted by _run)
        assert tf._run(ctx, und, False, 0, 1e300)["iters"] == 1


# ---- sweeps ----------------------------------------------------------------------------------------------------------------------
EMPTY = ([], [], np.zeros((0, 2), np.int64), [], np.zeros((0, 0)))


@BOTH
def test_exact_sweep_on_32_cus_matches_stepwise(ctx, directed):
    """tests/test_gpu_parity.py::test_fit_persistent_kernel_matches_stepwise_and_oracle under knob 32: every alpha's fit is an
    NSB = 2 launch (n = 700: Nt = 11, n = 640: Nt = 10)."""
    import cge.jl_amd as cg
    from cge.jl_amd import api, synth

    n = 640 if directed else 700
    assert api.fit_dir_geometry_test(n, 32) == (32, 4, 2)
    g = synth.abcd_like(n, 6 * n, max(2, n // 60), 8, seed=n, directed=directed)
    ctx.set_graph(g["edges"], g["eweights"], n)
    if directed:
        p1, ni, nj = api.draw_samples(ctx, 5, 2000, directed=True)
        smp = (p1, ni, nj, api.draw_samples(ctx, 6, 2000, directed=True)[0])
    else:
        smp = api.draw_samples(ctx, 11, 2000)
    args = (g["edges"], g["eweights"], g["comm"], g["embedding"], np.zeros(n), g["vweights"], *EMPTY, False)
    score = cg.wGCL_directed if directed else cg.wGCL
    out = {}
    with _knob(ctx, 32):
        try:
            for mode in (1, 2, 3):  # one launch (pair) per iteration / persistent, twice
                ctx.set_option("fit_persistent", min(mode, 2))
                out[mode] = score(*args, samples=smp, trace=True, ctx=ctx)
                assert (ctx.get_stat("fit_persistent_alphas") > 0) == (mode >= 2)
                assert ctx.get_stat("fit_persistent_fallbacks") == 0
        finally:
            ctx.set_option("fit_persistent", 0)
    (r1, t1), (r2, t2), (r3, t3) = out[1], out[2], out[3]
    assert t1["iters"] == t2["iters"] == t3["iters"]
    assert np.array_equal(r2, r3) and np.array_equal(t2["div"], t3["div"], equal_nan=True)
    assert np.allclose(r1, r2, rtol=1e-11, atol=1e-13)
    assert np.allclose(t1["div"], t2["div"], rtol=1e-11, equal_nan=True)


def test_landmark_score_on_32_cus_is_not_fused_and_agrees(ctx):
    from cge.jl_amd import api, synth

    g = synth.abcd_like(5000, 50000, 10, 16, seed=17)
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    ctx.set_embedding(g["embedding"])
    kw = dict(forced=4, method="rss", seed=3, auc_samples=5000)
    r0 = ctx.score(g["clusters"], 600, **kw)
    t0, N = ctx.last_trace, ctx.landmarks_info()[0]
    fused0 = ctx.get_stat("fit_fused_alphas")
    assert api.fit_dir_geometry_test(N, 32) == (32, 4, 2), N
    if tf._cus() >= 4 * ((N + 63) // 64):
        assert fused0 > 0  # knob 0: the fused geometry
    with _knob(ctx, 32):
        r1 = ctx.score(g["clusters"], 600, **kw)
        t1 = ctx.last_trace
        assert ctx.get_stat("fit_fused_alphas") == 0 and ctx.get_stat("fit_persistent_alphas") == t1["n_alpha"] > 0
        assert np.array_equal(r1, ctx.score(g["clusters"], 600, **kw))
    print("  600 landmarks, knob 32 against knob 0: same bits" if np.array_equal(r0, r1) else
          "  600 landmarks, knob 32 against knob 0: largest relative difference %.3g" % np.max(np.abs(r1 - r0) / np.maximum(np.abs(r0), 1e-300)))
    assert t0["iters"] == t1["iters"] and r0[0] == r1[0] and r0[4] == r1[4]
    assert np.allclose(r0, r1, rtol=1e-11, atol=1e-13)


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def _pack(Ns, cus):
    import ctypes as C

    from cge.jl_amd import api

    L = api.load_library()
    N = np.ascontiguousarray(Ns, dtype=np.int64)
    out = np.full(len(N), -2, np.int32)
    L.cge_batch_pack_test.restype = C.c_int
    L.cge_batch_pack_test.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    return L.cge_batch_pack_test(N.ctypes.data, len(N), int(cus), out.ctypes.data), out.tolist()


@BOTH
def test_batch_of_five_at_256_landmarks_on_32_cus(ctx, directed):
    """G = 16 = cus / 2: two members per launch group, three groups."""
    from cge.jl_amd import api, synth
    from test_gpu_batch import _assert_same, _embeddings, _separate

    assert api.fit_dir_geometry_test(256, 32) == (16, 4, 1)
    assert _pack([256] * 5, 32) == (3, [0, 0, 1, 1, 2])
    assert api.batch_pack_dir_test([256] * 5, 32)[1].tolist() == [0, 0, 1, 1, 2]
    g = synth.abcd_like(4000, 40000, 10, 16, seed=23, directed=directed)
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    embs = _embeddings(g, 5, seed=1)
    kw = dict(forced=4, method="rss", directed=directed, seed=5, auc_samples=6000)
    with _knob(ctx, 32):
        got = ctx.score_batch(embs, g["clusters"], 256, **kw)
        got_tr = ctx.last_traces
        launches, alphas = ctx.get_stat("fit_batched_launches"), ctx.get_stat("fit_batched_alphas")
        assert ctx.landmarks_info()[0] == 256
        exp, exp_tr = _separate(ctx, embs, g["clusters"], 256, **kw)
    _assert_same(got, got_tr, exp, exp_tr)
    n_alpha = [t["n_alpha"] for t in exp_tr]
    print("  n_alpha", n_alpha, "launches", launches, "member-alphas", alphas)
    assert launches > 0 and alphas == sum(n_alpha)
    assert launches >= max(n_alpha[:2]) + max(n_alpha[2:4]) + n_alpha[4]  # three groups: never five members in a launch
