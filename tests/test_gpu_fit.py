"""The Chung-Lu fixed point (src/divergence.jl:150-168, :434-467) iterate by iterate, in every form the sweep runs it by (run with
-m gpu on an MI355X).

The forms go through the testing hook cge_fit_test (the sweep's own fit functions, launch wrappers and geometry): 1 one launch
(pair) per iteration -- upper tiles, or symv_dir + update_dir; 2 the same on the packed tiles; 3 persistent, reading GD
(fit_flow_kernel / fit_flow_dir_kernel); 4 the fused instance (GD made in the prologue); 5 fit_flow_multi_kernel; 0 what a sweep
picks.  The reference is tests/fit_ref.py (np.longdouble, pinned on the CPU by tests/test_fit_ref.py), always on the power matrix
the hook returned, so the power's own error (tests/test_gpu_parity.py) stays out.  Which N sits on which geometry is derived from
the device's CU count with flow_geometry's formulas; the sizes are those of 256 CUs:

  1 .. 130      one to three tiles, odd and even-but-not-multiple-of-8 N (the guarded against the 16-byte loads of
                fit_symtile_kernel), a last tile one row wide, workgroups with a quarter block but no tile
  1985          Nt = 32, the first N with more workgroups than quarter blocks (tile workgroups that leave by the end mark)
  2816 / 2817   the last N on 4 waves per workgroup, the first on 8
  4032 / 4033   the last N of the persistent forms, the first they refuse (form 0 then runs form 1)
  4097          form 1 alone: Nt = 65

V1  exact inputs (D in {0, 1/4, .., 1} at alpha 1, start in {0.5, 1, 1.5, 2}, w = S r with r in {1/2, 1, 3/2, 2}): every product,
    sum, quotient and the move are exact in fp64 in any order, so with delta = 2 f_0 every form returns iters == 1 and T_1 bit for
    bit -- zero-degree rows of the directed fit their start value;
V2  one step on random inputs against long double within the a-priori bound of fit_ref.step_bound (2e-14 relative at N = 130,
    1e-12 at N = 4032; a dropped term of a row is 1 / N of it), with NaN in every element of D below its diagonal tile
    (undirected), which must not change a bit;
V3  K steps to a chosen end (delta between f_{K-1} and the smallest earlier f, a factor >= 1.1 from both): iters == K of every
    form, T_K within A_K times the one-step bound, A_K = max(2, 2 E64(K) / E64(1)) measured on the plain fp64 iteration;
V4  bits across forms where the kernels' comments promise them: 1 == 2, 4 == 3 under pow_exp2, every member of a form-5 launch ==
    its own form-4 launch, every form == itself on a second run and (3-5) under a start skew of 20 naps;
V5  the give-up path under fit_persistent_test_timeout, and every refusal of the hook by its message.

Measured on an MI355X (256 CUs; `-s` prints the figures):
  A_K: 2.0 .. 5.73 undirected (K = 1 .. 45; the largest at N = 700, K = 8), 2.0 .. 2.56 directed (K = 2 .. 13).
  Largest device error as a fraction of its tolerance, over all forms and sizes: V2 0.096 undirected, 0.12 directed;
  V3 0.049 undirected, 0.021 directed.
Scratch mutants of the kernels (not committed) and what noticed them: the guarded loads of fit_symtile_kernel dropping the last
column -- V1, V2, V3 at every N that takes that path; fit_flow_dir_kernel without the deg_in > 0 guard -- V1, V2, V3 directed;
epsilon decayed at every check -- V3 directed alone (N <= 700, where some iteration goes without a decay); a reducer of
fit_flow_kernel leaving out one of its sixteen partial sums -- V1, V2, V3 from N = 1985 on (the sizes with 16 tiles per row).
"""
import functools

import numpy as np
import pytest

import fit_ref as fr

pytestmark = pytest.mark.gpu

LD = fr.LD
SMALL = [1, 2, 7, 63, 64, 65, 66, 72, 127, 128, 129, 130]
BIG = [1985, 2816, 2817, 4032, 4097]
REFUSED = 4033  # (on 256 CUs)
E_ARG = -7


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


def _geometry(N, cus=None):
    """flow_geometry (kernels_fitp.hip): (G, NW, every workgroup has at most one quarter block) or None = declined.  cus: the
    CU count the context is told (knob test_device_cus: tests/test_gpu_small_chip_fits.py); None = the device's own."""
    cus = cus or _cus()
    Nt = (N + 63) // 64
    NT = Nt * (Nt + 1) // 2
    NW = 4 if NT <= 4 * cus else 8
    G = min(cus, max((NT + NW - 1) // NW, 4 * Nt))
    tpw = (NT + NW * G - 1) // (NW * G)
    if tpw > 1 or Nt > 64 or 4 * Nt > 2 * G:
        return None
    return G, NW, 4 * Nt <= G


def _forms(N, directed, with_auto=True, cus=None):
    g = _geometry(N, cus)
    forms = ([0] if with_auto else []) + [1]
    if not directed:
        forms.append(2)
    if g:
        forms.append(3)
    if g and g[2] and not directed:
        forms += [4, 5]
    return forms


def _expected(N, form, cus=None):
    """The form that runs: form 0 is the persistent one from 128 vertices on where the geometry applies."""
    if form:
        return form
    return 3 if N >= 128 and _geometry(N, cus) else 1


def test_the_sizes_reach_what_they_are_chosen_for():
    if _cus() != 256:
        return  # (the table of the module docstring is that of 256 CUs; every other test derives its forms from the CU count)
    g = {N: _geometry(N) for N in SMALL + BIG + [REFUSED, 1984]}
    assert all(g[N] and g[N][2] and g[N][1] == 4 for N in SMALL)
    assert g[130][0] == 12 and g[1984][0] == 4 * 31 and g[1985][0] == 132 > 4 * 32  # workgroups without a quarter block
    assert g[2816][1] == 4 and g[2817][1] == 8
    assert g[4032] and g[REFUSED] is None and g[4097] is None and (4097 + 63) // 64 == 65


def _run(ctx, pr, directed, form, delta, eps=None, want_GD=False, cus=None):
    ran, (out,) = ctx.fit_test(pr, directed=directed, form=form, eps=eps, delta=delta, want_GD=want_GD)
    N = pr["D"].shape[0]
    assert ran == _expected(N, form, cus), (N, directed, form, ran)
    return out


def _same(a, b):
    return a["iters"] == b["iters"] and a["status"] == b["status"] and np.array_equal(a["T"], b["T"], equal_nan=True) and (
        a["Tb"] is None or np.array_equal(a["Tb"], b["Tb"], equal_nan=True))


def _device_gd(ctx, pr, directed):
    """The full symmetric power matrix the forms read, as the hook's launches made it."""
    out = _run(ctx, pr, directed, 1, 1e300, want_GD=True)
    assert out["iters"] == 1
    GD = out["GD"]
    if directed:
        assert np.array_equal(GD, GD.T)
        return GD
    N = GD.shape[0]
    below = np.arange(N)[None, :] < (np.arange(N)[:, None] // 64) * 64
    assert np.all(np.isnan(GD[below])) and not np.any(np.isnan(GD[~below]))  # the upper tiles, and nothing else
    return fr.symmetric(GD)


def _nan_below_the_diagonal_tiles(D):
    N = D.shape[0]
    D = D.copy()
    D[np.arange(N)[None, :] < (np.arange(N)[:, None] // 64) * 64] = np.nan
    return D


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    print(f"  {key}: largest error / tolerance so far {_worst[key]:.3g}")


# ---- V1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("N", SMALL + BIG + [REFUSED])
def test_exact_inputs_give_the_fp64_step_bit_for_bit(ctx, N, directed):
    pr, T1, f0 = fr.exact_problem(N, 40 + N, directed)
    eps = 0.5 if directed else 0.25
    g = _run(ctx, pr, directed, 1, 2.0 * f0, eps=eps, want_GD=True)["GD"]
    keep = np.ones((N, N), bool) if directed else np.arange(N)[None, :] >= (np.arange(N)[:, None] // 64) * 64
    assert np.array_equal(g[keep], (1.0 - pr["D"])[keep])  # the power at alpha = 1 is exact on these values
    for form in _forms(N, directed):
        out = _run(ctx, pr, directed, form, 2.0 * f0, eps=eps)
        assert out["iters"] == 1 and out["status"] == 0, (N, form, out["iters"], out["status"])
        if directed:
            assert np.array_equal(out["T"], T1[0]) and np.array_equal(out["Tb"], T1[1]), (N, form)
            if N >= 8:  # zero-degree rows come back as they started
                assert np.array_equal(out["T"][[1, 3]], pr["T0"][[1, 3]]) and np.array_equal(out["Tb"][[2, 5]], pr["T0b"][[2, 5]])
        else:
            bad = np.flatnonzero(out["T"] != T1)
            assert bad.size == 0, (N, form, bad[:8], out["T"][bad[:8]], T1[bad[:8]])


# ---- V2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SMALL + BIG)
def test_one_step_undirected_within_the_a_priori_bound(ctx, N):
    alpha = (1.0, 4.0, 10.0, 0.25)[N % 4]
    pr = fr.random_undirected(N, alpha, 300 + N)
    pr["T0"] = np.exp(0.3 * np.random.default_rng(N).normal(size=N))
    GD = _device_gd(ctx, pr, False)
    ref = fr.fit_undirected(GD, pr["T0"], pr["w"], 0.25, steps=1)
    tol = fr.step_bound(0.25, pr["T0"], pr["w"], ref["S"][0], ref["T"][1], N)
    delta = 2.0 * float(ref["f"][0])
    dirty = dict(pr, D=_nan_below_the_diagonal_tiles(pr["D"]))
    for form in _forms(N, False):
        out = _run(ctx, dirty, False, form, delta)
        assert out["iters"] == 1 and out["status"] == 0, (N, form)
        err = np.abs(LD(out["T"]) - ref["T"][1])
        assert np.all(err <= tol), (N, form, int(np.argmax(err / tol)), float(np.max(err / tol)))
        _note("V2 undirected", np.max(err / tol))
        if N <= 700:  # what lies below the diagonal tiles is never read: the same bits from the whole matrix
            assert _same(out, _run(ctx, pr, False, form, delta)), (N, form)


@pytest.mark.parametrize("N", SMALL + BIG)
def test_one_step_directed_within_the_a_priori_bound(ctx, N):
    alpha = (1.0, 4.0, 10.0, 0.25)[N % 4]
    pr = fr.random_directed(N, alpha, 400 + N)
    rng = np.random.default_rng(N)
    pr["T0"], pr["T0b"] = np.exp(0.3 * rng.normal(size=N)), np.exp(0.3 * rng.normal(size=N))  # (zero-degree rows too: kept)
    GD = _device_gd(ctx, pr, True)
    ref = fr.fit_directed(GD, pr["T0"], pr["T0b"], pr["w"], pr["w2"], 0.9, steps=1)
    delta = 2.0 * float(ref["f"][0])
    for form in _forms(N, True):
        out = _run(ctx, pr, True, form, delta)
        assert out["iters"] == 1 and out["status"] == 0, (N, form)
        for got, k, start, deg in ((out["T"], 0, pr["T0"], pr["w"]), (out["Tb"], 1, pr["T0b"], pr["w2"])):
            z = deg == 0
            assert np.array_equal(got[z], start[z]), (N, form, k)
            tol = fr.step_bound(0.9, start, deg, ref["S"][0][k], ref["T"][1][k], N)
            err = np.abs(LD(got) - ref["T"][1][k])
            assert np.all(err[~z] <= tol[~z]), (N, form, k, float(np.max(err[~z] / tol[~z])))
            _note("V2 directed", np.max(err[~z] / tol[~z]))


# ---- V3 --------------------------------------------------------------------------------------------------------------
_case_cache = {}


def _cases(ctx, N, directed):
    """The chain of N (tests/fit_ref.py) with long-double references on the device's own power matrices; computed once."""
    if (N, directed) not in _case_cache:
        _case_cache[N, directed] = fr.chain_cases(N, directed, lambda pr, alpha: _device_gd(ctx, pr, directed))
    return _case_cache[N, directed]


def _check_case(ctx, c, N, directed, forms, cus=None, tag=""):
    """Every form ends the case at iters == K with T_K within A_K times the one-step bound.  Returns the outputs by form."""
    pr, K, ref = c["problem"], c["K"], c["ref"]
    assert c["gap"] >= fr.GAP  # from the reference alone: no form is exempted from iters == K
    outs = {}
    for form in forms:
        out = outs[form] = _run(ctx, pr, directed, form, c["delta"], cus=cus)
        assert out["iters"] == K and out["status"] == 0, (N, directed, form, out["iters"], K)
        pairs = [(out["T"], ref["T"][K - 1], ref["T"][K], ref["S"][K - 1], pr["w"])] if not directed else [
            (out["T"], ref["T"][K - 1][0], ref["T"][K][0], ref["S"][K - 1][0], pr["w"]),
            (out["Tb"], ref["T"][K - 1][1], ref["T"][K][1], ref["S"][K - 1][1], pr["w2"])]
        for got, Tp, Tn, Sp, deg in pairs:
            live = (deg > 0) if directed else np.ones(N, bool)
            assert np.array_equal(LD(got[~live]), Tn[~live])
            tol = c["A"] * fr.step_bound(ref["eps"][K - 1], Tp, deg, Sp, Tn, N)
            err = np.abs(LD(got) - Tn)
            assert np.all(err[live] <= tol[live]), (N, directed, form, K, float(np.max(err[live] / tol[live])), c["A"])
            _note(("V3 directed" if directed else "V3 undirected") + tag, np.max(err[live] / tol[live]))
    return outs


@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("N", sorted(fr.UNDIRECTED_CHAINS))
def test_k_steps_to_a_chosen_end(ctx, N, directed):
    cases = _cases(ctx, N, directed)
    print(f"  N = {N}: K, A_K =", [(c["K"], round(c["A"], 2)) for c in cases])
    assert sum(c["start"] == "prev" for c in cases) * 2 >= len(cases)  # starts that are not the sweep's, as a sweep has them
    if directed and N == fr.DESIGNATED_DIRECTED:
        c = cases[0]
        assert len(c["decays"]) >= 3 and len(c["decays"]) < c["K"] - 1  # epsilon decays, and not at every iteration
    if not directed and N == 65:
        assert cases[1]["K"] == 1 and not np.all(cases[1]["problem"]["T0"] == 1.0)  # ends at once from a non-trivial start
        assert {c["K"] % 12 for c in cases} == set(range(12))  # every residue of the rings of 2, 3 and 4
    for c in cases:
        _check_case(ctx, c, N, directed, _forms(N, directed, with_auto=False))


# ---- V4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", sorted(fr.UNDIRECTED_CHAINS))
def test_bits_across_forms_where_the_kernels_promise_them(ctx, N):
    """kernels_fitp.hip: the packed tiles do "the same FMAs and additions" (1 == 2); the fused prologue's power is
    exp2_matrix_upper_kernel's "own function and bits" (4 == 3 under pow_exp2 = 1, the default); a member of
    fit_flow_multi_kernel has "the arithmetic of its own fit_flow_kernel<1, NW, true, 1> launch" (5 == 4)."""
    forms = _forms(N, False, with_auto=False)
    for c in _cases(ctx, N, False)[:4]:
        o = {f: _run(ctx, c["problem"], False, f, c["delta"]) for f in forms}
        assert _same(o[1], o[2]), (N, c["K"])
        if 4 in forms:
            assert _same(o[4], o[3]) and _same(o[5], o[4]), (N, c["K"])


def test_members_of_a_multi_launch_match_their_own_fused_launch(ctx):
    prs = [fr.random_undirected(n, a, 500 + n) for n, a in ((65, 1.0), (300, 4.0), (700, 10.0))]
    gs = [_geometry(p["D"].shape[0]) for p in prs]
    if not (all(g and g[2] for g in gs) and len({g[1] for g in gs}) == 1 and sum(g[0] for g in gs) <= _cus()):
        return  # (a device on which the three do not share a launch: the refusals are tested below)
    ran, outs = ctx.fit_test(prs, form=5, delta=1e-3)
    assert ran == 5
    iters = [o["iters"] for o in outs]
    assert all(o["status"] == 0 for o in outs) and min(iters) > 30, iters
    for p, o in zip(prs, outs):
        assert _same(o, _run(ctx, p, False, 4, 1e-3))
    ran, again = ctx.fit_test(prs[::-1], form=5, delta=1e-3)  # (other slots, other workgroups)
    assert all(_same(a, b) for a, b in zip(again[::-1], outs))


@pytest.mark.parametrize("N", [130, 700, 2817])
def test_every_form_repeats_itself_also_under_a_start_skew(ctx, N):
    for directed in (False, True):
        c = _cases(ctx, N, directed)[1]
        forms = _forms(N, directed)
        first = {f: _run(ctx, c["problem"], directed, f, c["delta"]) for f in forms}
        for f in forms:
            assert first[f]["iters"] == c["K"] and _same(first[f], _run(ctx, c["problem"], directed, f, c["delta"])), (N, directed, f)
        try:
            ctx.set_option("fit_persistent_test_delay", 20)
            for f in forms:
                if f >= 3:
                    assert _same(first[f], _run(ctx, c["problem"], directed, f, c["delta"])), (N, directed, f, "delay")
        finally:
            ctx.set_option("fit_persistent_test_delay", 0)


# ---- V5 --------------------------------------------------------------------------------------------------------------
def test_an_abandoned_persistent_launch_writes_nothing(ctx):
    N = 130
    und, drc = _cases(ctx, N, False)[1], _cases(ctx, N, True)[1]
    starts = {k: v.copy() for k, v in list(und["problem"].items()) + [("d" + k, v) for k, v in drc["problem"].items()]
              if isinstance(v, np.ndarray)}
    want_u, want_d = _run(ctx, und["problem"], False, 1, und["delta"]), _run(ctx, drc["problem"], True, 1, drc["delta"])
    try:
        ctx.set_option("fit_persistent_test_timeout", 1)
        for form in (3, 4, 5):
            ran, (out,) = ctx.fit_test(und["problem"], form=form, delta=und["delta"])
            assert ran == form and out["status"] == 1 and np.all(np.isnan(out["T"])), (form, out["status"], out["T"][:4])
        # directed: Tin / Tout are updated in place and on success only -- the device still holds the start
        ran, (out,) = ctx.fit_test(drc["problem"], directed=True, form=3, delta=drc["delta"])
        assert ran == 3 and out["status"] == 1
        assert np.array_equal(out["T"], drc["problem"]["T0"]) and np.array_equal(out["Tb"], drc["problem"]["T0b"])
        # form 0: the sweep's fallback, one launch (pair) per iteration from the same start
        ran, (out,) = ctx.fit_test(und["problem"], form=0, delta=und["delta"])
        assert ran == 1 and _same(out, want_u)
        ran, (out,) = ctx.fit_test(drc["problem"], directed=True, form=0, delta=drc["delta"])
        assert ran == 1 and _same(out, want_d)
    finally:
        ctx.set_option("fit_persistent_test_timeout", 0)
    for k, v in list(und["problem"].items()) + [("d" + k, v) for k, v in drc["problem"].items()]:
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, starts[k])  # the caller's vectors: unchanged
    assert _same(_run(ctx, und["problem"], False, 3, und["delta"]), _run(ctx, und["problem"], False, 0, und["delta"]))  # and back


# ---- the refusals ------------------------------------------------------------------------------------------------------
def _refused(ctx, text, *args, **kw):
    from cge.jl_amd import api

    with pytest.raises(api.CGEError) as e:
        ctx.fit_test(*args, **kw)
    assert e.value.code == E_ARG and "fit_test" in str(e.value) and text in str(e.value), str(e.value)


def test_refusals(ctx):
    small = fr.random_undirected(65, 1.0, 1)
    dsmall = fr.random_directed(65, 1.0, 1)
    for form in (2, 4, 5):
        _refused(ctx, "undirected only", dsmall, directed=True, form=form)
    _refused(ctx, "form 5 only", [small, small], form=3)
    _refused(ctx, "at most 16", [small] * 17, form=5)
    N = next(n for n in range(64, 64 * 66, 64) if _geometry(n + 1) is None) + 1  # the first N the persistent forms decline
    assert _cus() != 256 or N == REFUSED
    big, dbig = fr.random_undirected(N, 1.0, 2), fr.random_directed(N, 1.0, 2)
    for form in (3, 4, 5):
        _refused(ctx, "declines N = %d" % N, big, form=form)
    _refused(ctx, "declines N = %d" % N, dbig, directed=True, form=3)
    assert _run(ctx, big, False, 0, 1e300)["iters"] == 1 and _run(ctx, dbig, True, 0, 1e300)["iters"] == 1  # (form 0 runs form 1)
    n4 = max(n for n in range(64, N, 64) if _geometry(n)[1] == 4)
    if _geometry(n4 + 1):  # problems on 4 and on 8 waves per workgroup
        _refused(ctx, "one NW", [small, fr.random_undirected(n4 + 1, 1.0, 3)], form=5)
    G = _geometry(700)[0]
    _refused(ctx, "workgroups in all", [fr.random_undirected(700, 1.0, 4)] * (_cus() // G + 1), form=5)
    try:
        ctx.set_option("pow_exp2", 0)
        for form in (4, 5):
            _refused(ctx, "pow_exp2", small, form=form)
    finally:
        ctx.set_option("pow_exp2", 1)
