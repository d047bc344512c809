"""The directed Chung-Lu fit by the tile pair (fit_symtile_dir_kernel + fit_symreduce_dir_kernel, kernels_fitp.hip), iterate by
iterate: forms 7 (row-major GD) and 8 (the packed tiles) of the testing hook cge_fit_test against tests/fit_ref.py (long double)
within fit_ref's a-priori bound, reached the way tests/test_gpu_fit.py reaches the iterates of directed form 1.

N: 63 (one ragged tile), 64, 65 (a last tile one row wide, odd N: the guarded loads), 129, 130 (three tiles per side, odd and
even-but-not-a-multiple-of-8), 256 (full tiles, the 16-byte loads), 321 (six tiles per side: the reducer adds more partial
vectors than it has waves).

V1  exact inputs: T_1 bit for bit, rows with deg_in = 0 or deg_out = 0 equal to their start;
V2  one step on random inputs within fit_ref.step_bound;
V3  the chains of fit_ref at every N that has a directed one (65, 130: epsilon decays, and not at every iteration): iters == K,
    T_K within A_K times the one-step bound;
V4  forms 7 and 8 agree bit for bit, and each with itself on a second run;
V5  form 8 undirected and form 7 with several problems are refused before any launch."""
import numpy as np
import pytest

import fit_dir_ref as fd
import fit_ref as fr

pytestmark = pytest.mark.gpu

LD = fr.LD
SIZES = [63, 64, 65, 129, 130, 256, 321]
E_ARG = -7


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _run(ctx, pr, form, delta, eps=None, want_GD=False):
    ran, (out,) = ctx.fit_test(pr, directed=True, form=form, eps=eps, delta=delta, want_GD=want_GD)
    assert ran == form, (form, ran)
    return out


def _same(a, b):
    return a["iters"] == b["iters"] and a["status"] == b["status"] and np.array_equal(a["T"], b["T"], equal_nan=True) and np.array_equal(
        a["Tb"], b["Tb"], equal_nan=True)


def _device_gd(ctx, pr):
    """The full symmetric power matrix the forms read, as the hook's launches made it."""
    out = _run(ctx, pr, 7, 1e300, want_GD=True)
    assert out["iters"] == 1
    assert np.array_equal(out["GD"], out["GD"].T)
    return out["GD"]


@pytest.mark.parametrize("N", SIZES)
def test_exact_inputs_give_the_fp64_step_bit_for_bit(ctx, N):
    pr, T1, f0 = fr.exact_problem(N, 40 + N, True)
    for form in (7, 8):
        out = _run(ctx, pr, form, 2.0 * f0, eps=0.5)
        assert out["iters"] == 1 and out["status"] == 0, (N, form, out["iters"], out["status"])
        assert np.array_equal(out["T"], T1[0]) and np.array_equal(out["Tb"], T1[1]), (N, form)
        assert np.array_equal(out["T"][[1, 3]], pr["T0"][[1, 3]]) and np.array_equal(out["Tb"][[2, 5]], pr["T0b"][[2, 5]])


@pytest.mark.parametrize("N", SIZES)
def test_one_step_within_the_a_priori_bound(ctx, N):
    alpha = (1.0, 4.0, 10.0, 0.25)[N % 4]
    pr = fr.random_directed(N, alpha, 400 + N)
    assert np.count_nonzero(pr["w"] == 0) == 2 and np.count_nonzero(pr["w2"] == 0) == 2
    rng = np.random.default_rng(N)
    pr["T0"], pr["T0b"] = np.exp(0.3 * rng.normal(size=N)), np.exp(0.3 * rng.normal(size=N))  # (zero-degree rows too: kept)
    GD = _device_gd(ctx, pr)
    ref = fr.fit_directed(GD, pr["T0"], pr["T0b"], pr["w"], pr["w2"], 0.9, steps=1)
    delta = 2.0 * float(ref["f"][0])
    outs = {}
    for form in (7, 8):
        out = outs[form] = _run(ctx, pr, form, delta)
        assert out["iters"] == 1 and out["status"] == 0, (N, form)
        for got, k, start, deg in ((out["T"], 0, pr["T0"], pr["w"]), (out["Tb"], 1, pr["T0b"], pr["w2"])):
            z = deg == 0
            assert np.array_equal(got[z], start[z]), (N, form, k)
            tol = fr.step_bound(0.9, start, deg, ref["S"][0][k], ref["T"][1][k], N)
            err = np.abs(LD(got) - ref["T"][1][k])
            print(f"  N = {N} form {form} side {k}: error / tolerance {float(np.max(err[~z] / tol[~z])):.3g}")
            assert np.all(err[~z] <= tol[~z]), (N, form, k, float(np.max(err[~z] / tol[~z])))
    assert _same(outs[7], outs[8]), N


_case_cache = {}


def _cases(ctx, N):
    if N not in _case_cache:
        _case_cache[N] = fr.chain_cases(N, True, lambda pr, alpha: _device_gd(ctx, pr))
    return _case_cache[N]


@pytest.mark.parametrize("N", [n for n in sorted(fr.DIRECTED_CHAINS) if n <= 700])
def test_k_steps_to_a_chosen_end(ctx, N):
    cases = _cases(ctx, N)
    print(f"  N = {N}: K, A_K =", [(c["K"], round(c["A"], 2)) for c in cases])
    if N == fr.DESIGNATED_DIRECTED:
        c = cases[0]
        assert len(c["decays"]) >= 3 and len(c["decays"]) < c["K"] - 1  # epsilon decays, and not at every iteration
    for c in cases:
        pr, K, ref = c["problem"], c["K"], c["ref"]
        assert c["gap"] >= fr.GAP
        outs = {}
        for form in (7, 8):
            out = outs[form] = _run(ctx, pr, form, c["delta"])
            assert out["iters"] == K and out["status"] == 0, (N, form, out["iters"], K)
            for got, s, deg in ((out["T"], 0, pr["w"]), (out["Tb"], 1, pr["w2"])):
                Tp, Tn, Sp = ref["T"][K - 1][s], ref["T"][K][s], ref["S"][K - 1][s]
                live = deg > 0
                assert np.array_equal(LD(got[~live]), Tn[~live])
                tol = c["A"] * fr.step_bound(ref["eps"][K - 1], Tp, deg, Sp, Tn, N)
                err = np.abs(LD(got) - Tn)
                print(f"  N = {N} K = {K} form {form} side {s}: error / tolerance {float(np.max(err[live] / tol[live])):.3g}")
                assert np.all(err[live] <= tol[live]), (N, form, K, float(np.max(err[live] / tol[live])), c["A"])
        assert _same(outs[7], outs[8]), (N, K)
        assert _same(outs[8], _run(ctx, pr, 8, c["delta"])), (N, K)  # and a second run repeats itself


@pytest.mark.parametrize("N", [256, 321])
def test_convergence_at_sizes_without_a_chain(ctx, N):
    """delta = 1e-3 from the sweep's start on a problem with a fixed point (tests/fit_dir_ref.py): the iteration count of the
    long-double reference -- more than one batch of launches, an epsilon decay on the way --, both forms the same bits."""
    pr = fd.consistent_directed(N, 4.0, 450 + N)
    GD = _device_gd(ctx, pr)
    ref = fr.fit_directed(GD, pr["T0"], pr["T0b"], pr["w"], pr["w2"], 0.9, delta=1e-3, max_iters=1000)
    K = ref["iters"]
    assert K > 32 and float(ref["f"][K - 1]) < 1e-3 / 1.1 and float(ref["f"][K - 2]) > 1e-3 * 1.1  # (the input condition)
    a, b = _run(ctx, pr, 7, 1e-3), _run(ctx, pr, 8, 1e-3)
    assert a["iters"] == K and a["status"] == 0, (a["iters"], K)
    assert _same(a, b)
    for got, s, deg in ((a["T"], 0, pr["w"]), (a["Tb"], 1, pr["w2"])):
        assert np.array_equal(got[deg == 0], np.zeros(2))  # zero-degree rows: their start


def test_refusals(ctx):
    from cge.jl_amd import api

    small, dsmall = fr.random_undirected(65, 1.0, 1), fr.random_directed(65, 1.0, 1)
    for form in (7, 8):
        with pytest.raises(api.CGEError) as e:
            ctx.fit_test(small, form=form)
        assert e.value.code == E_ARG and "directed only" in str(e.value), str(e.value)
    with pytest.raises(api.CGEError) as e:
        ctx.fit_test([dsmall, dsmall], directed=True, form=7)
    assert e.value.code == E_ARG and "form 5 only" in str(e.value), str(e.value)
