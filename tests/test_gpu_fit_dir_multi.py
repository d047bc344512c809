"""Several directed Chung-Lu fits in one launch (fit_flow_dir_multi_kernel, kernels_fitp.hip) through form 6 of the testing hook
cge_fit_test (run with -m gpu on an MI355X).

A member of a shared launch keeps the geometry (G, NW), the slots and the arithmetic of its own fit_flow_dir_kernel launch, so
its iterate, its iteration count and its status are those of form 3 bit for bit -- whatever the other members are, in whichever
order, on a second run and under a start skew.  The kernel is also held to the long-double reference directly (tests/fit_ref.py,
the cases and the criterion of tests/test_gpu_fit.py), so that it is not tied to the reference through form 3 alone.  Which N
sits on which geometry is derived from the device's CU count with the formulas of flow_geometry, as test_gpu_fit.py
does (the one geometry of every persistent fit); on 256 CUs: N = 65 -> G = 8, 300 -> 20, 700 -> 44, NW = 4 up to
N = 2816, and no N whose workgroups would reduce two quarter blocks.
"""
import numpy as np
import pytest

import fit_ref as fr
import test_gpu_fit as tgf

pytestmark = pytest.mark.gpu

_geometry, _same, _cus = tgf._geometry, tgf._same, tgf._cus


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _feasible(N, alpha, seed):
    """fr.random_directed with degrees that HAVE a fixed point: the sums of a hidden (Tin, Tout) that is 0 where the degree is, so
    that the sweep's epsilon = 0.9 and delta = 1e-3 end the fit (in 35 .. 60 iterations from the sweep's start, in long double
    as in fp64).  The perturbed degrees of random_directed have sum(deg_in) != sum(deg_out): no fixed point, and a fit with
    delta = 1e-3 never ends on them -- test_gpu_fit.py picks a delta per case for that reason; a shared launch has one delta."""
    pr = fr.random_directed(N, alpha, seed)
    rng = np.random.default_rng(seed + 5)
    GD = (1.0 - pr["D"]) ** alpha
    Ti, To = np.exp(0.5 * rng.normal(size=N)) * (pr["w"] > 0), np.exp(0.5 * rng.normal(size=N)) * (pr["w2"] > 0)
    d = np.diagonal(GD)
    pr["w"], pr["w2"] = Ti * (GD @ To + d * To), To * (GD @ Ti + d * Ti)
    assert np.array_equal(pr["w"] > 0, pr["T0"] > 0) and np.array_equal(pr["w2"] > 0, pr["T0b"] > 0)
    return pr


@pytest.fixture(scope="module")
def three():
    """Three problems of different N and alpha; each has two rows of in-degree 0 and two others of out-degree 0."""
    prs = [_feasible(n, a, 600 + n) for n, a in ((65, 1.0), (300, 4.0), (700, 10.0))]
    for p in prs:
        assert np.sum(p["w"] == 0) == 2 and np.sum(p["w2"] == 0) == 2
    return prs


def _shares_a_launch(prs):
    gs = [_geometry(p["D"].shape[0]) for p in prs]
    return all(g and g[2] for g in gs) and len({g[1] for g in gs}) == 1 and sum(g[0] for g in gs) <= _cus()


def _own(ctx, pr, delta=1e-3):
    ran, (out,) = ctx.fit_test(pr, directed=True, form=3, delta=delta)
    assert ran == 3
    return out


def test_members_equal_their_own_launch_in_any_order_again_and_under_a_start_skew(ctx, three):
    if not _shares_a_launch(three):
        return  # (a device on which the three do not share a launch: the refusals are tested below)
    own = [_own(ctx, p) for p in three]
    iters = [o["iters"] for o in own]
    assert all(o["status"] == 0 for o in own) and min(iters) > 3 and len(set(iters)) > 1, iters
    ran, outs = ctx.fit_test(three, directed=True, form=6, delta=1e-3)
    assert ran == 6
    for p, o, w in zip(three, outs, own):
        assert _same(o, w), (p["D"].shape[0], o["iters"], w["iters"])
        assert np.array_equal(o["T"][p["w"] == 0], p["T0"][p["w"] == 0]) and np.array_equal(o["Tb"][p["w2"] == 0], p["T0b"][p["w2"] == 0])
    ran, rev = ctx.fit_test(three[::-1], directed=True, form=6, delta=1e-3)  # (other slots, other workgroups)
    assert all(_same(a, b) for a, b in zip(rev[::-1], own))
    ran, again = ctx.fit_test(three, directed=True, form=6, delta=1e-3)
    assert all(_same(a, b) for a, b in zip(again, own))
    try:
        ctx.set_option("fit_persistent_test_delay", 20)
        ran, late = ctx.fit_test(three, directed=True, form=6, delta=1e-3)
    finally:
        ctx.set_option("fit_persistent_test_delay", 0)
    assert all(_same(a, b) for a, b in zip(late, own))


def test_the_eight_wave_instance_equals_its_own_launch(ctx):
    cands = [n for n in range(64, 64 * 64 + 1, 64) if _geometry(n + 1) and _geometry(n + 1)[1] == 8 and _geometry(n + 1)[2]]
    if not cands:
        return  # (no N on eight waves with one quarter block per workgroup on this device)
    N = cands[0] + 1
    assert _cus() != 256 or N == 2817
    pr = _feasible(N, 1.0, 77)
    ran, (out,) = ctx.fit_test(pr, directed=True, form=6, delta=1e-3)
    assert ran == 6 and out["status"] == 0 and out["iters"] > 3
    assert _same(out, _own(ctx, pr))


@pytest.mark.parametrize("N", [65, 130, 700])
def test_a_lone_member_against_the_long_double_reference(ctx, N):
    """iters == K exactly and T_K within A_K times the a-priori one-step bound: _check_case's criterion, on the chain's first case
    (at N = 130 the designated one, with epsilon decays at some iterations and not at others)."""
    c = tgf._cases(ctx, N, True)[0]
    assert c["K"] >= 2
    tgf._check_case(ctx, c, N, True, [6])


def test_an_abandoned_launch_returns_every_start(ctx, three):
    if not _shares_a_launch(three):
        return
    try:
        ctx.set_option("fit_persistent_test_timeout", 1)
        ran, outs = ctx.fit_test(three, directed=True, form=6, delta=1e-3)
    finally:
        ctx.set_option("fit_persistent_test_timeout", 0)
    assert ran == 6
    for p, o in zip(three, outs):
        assert o["status"] == 1 and np.array_equal(o["T"], p["T0"]) and np.array_equal(o["Tb"], p["T0b"])
    ran, outs = ctx.fit_test(three, directed=True, form=6, delta=1e-3)  # and back
    assert all(o["status"] == 0 for o in outs)


def test_sixteen_members_in_one_launch(ctx):
    G = _geometry(65)[0]
    n = min(16, _cus() // G)
    assert _cus() != 256 or n == 16
    prs = [_feasible(65, 1.0 + 0.25 * k, 900 + k) for k in range(n)]
    ran, outs = ctx.fit_test(prs, directed=True, form=6, delta=1e-3)
    assert ran == 6
    for k in (0, n // 2, n - 1):
        assert _same(outs[k], _own(ctx, prs[k])), k
    assert all(o["status"] == 0 and o["iters"] > 0 for o in outs)


def _refused(ctx, text, *args, **kw):
    from cge.jl_amd import api

    with pytest.raises(api.CGEError) as e:
        ctx.fit_test(*args, **kw)
    assert e.value.code == tgf.E_ARG and "fit_test" in str(e.value) and text in str(e.value), str(e.value)


def test_refusals(ctx):
    small, usmall = fr.random_directed(65, 1.0, 1), fr.random_undirected(65, 1.0, 1)
    _refused(ctx, "form 6 is directed only", usmall, form=6)
    _refused(ctx, "form 6 is directed only", [usmall, usmall], form=6)
    _refused(ctx, "form 6 takes at most 16", [small] * 17, directed=True, form=6)
    N = next(n for n in range(64, 64 * 66, 64) if _geometry(n + 1) is None) + 1  # the first N the persistent forms decline
    _refused(ctx, "declines N = %d" % N, fr.random_directed(N, 1.0, 2), directed=True, form=6)
    two = [n for n in range(1, N) if _geometry(n) and not _geometry(n)[2]]  # workgroups with two quarter blocks (none on 256 CUs)
    if two:
        _refused(ctx, "one quarter block per workgroup", fr.random_directed(two[0], 1.0, 3), directed=True, form=6)
    n4 = max(n for n in range(64, N, 64) if _geometry(n)[1] == 4)
    if _geometry(n4 + 1) and _geometry(n4 + 1)[2]:  # problems on 4 and on 8 waves per workgroup
        _refused(ctx, "form 6 takes problems of one NW", [small, fr.random_directed(n4 + 1, 1.0, 3)], directed=True, form=6)
    G = _geometry(700)[0]
    _refused(ctx, "problems of form 6 need", [fr.random_directed(700, 1.0, 4)] * (_cus() // G + 1), directed=True, form=6)
    # the refusals of the forms beside it keep their texts
    _refused(ctx, "undirected only", small, directed=True, form=5)
    _refused(ctx, "form 5 only", [small, small], directed=True, form=3)
