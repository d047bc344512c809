"""Whole exact sweeps in the packed form (option "exact_packed": the upper tiles of the current alpha's GD are the only O(N^2)
device storage): against the oracle, against the resident form bit for bit, the footprint, the auto rule and its refusal, the
shapes the form does not apply to, and buffers left by an earlier resident sweep."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's tolerance against the oracle (tests/test_gpu_parity.py)
EMPTY = ([], [], np.zeros((0, 2), np.int64), [], np.zeros((0, 0)))
CGE_E_OOM = -6


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


def _cmp_result(res, exp, tr, etr):  # the assertions of tests/test_gpu_parity.py::_cmp_result
    assert len(res) == len(exp)
    assert res[0] == exp[0] and res[4] == exp[4], (res, exp)  # best alphas
    assert np.allclose(res, exp, rtol=RTOL, atol=1e-12), (res, exp)
    assert tr["iters"] == etr["iters"], "Chung-Lu iteration counts differ"
    assert np.allclose(tr["div"], etr["div"], rtol=RTOL, equal_nan=True)
    assert np.allclose(tr["auc"], etr["auc"], rtol=RTOL, atol=1e-12, equal_nan=True)


def _inputs(ctx, n, C, d, seed, weighted=False, split=False, n_sets=1, diag=False, directed=False, S=800):
    """A synthetic graph, its samples (drawn once, handed to both sides) and the wGCL argument tuple."""
    from cge.jl_amd import api, synth

    g = synth.abcd_like(n, 5 * n, C, d, seed=seed, directed=directed)
    rng = np.random.default_rng(seed)
    ew, vw = g["eweights"], g["vweights"]
    if weighted:  # dyadic weights: every weight sum is exact in any order
        ew = rng.integers(1, 9, size=len(ew)) / 2.0
        vw = np.zeros(n)
        np.add.at(vw, g["edges"][:, 0] - 1, ew)
        np.add.at(vw, g["edges"][:, 1] - 1, ew)
    ctx.set_graph(g["edges"], ew, n)
    if directed:
        p1, ni, nj = api.draw_samples(ctx, seed, S, directed=True, n_sets=n_sets)
        p2, _, _ = api.draw_samples(ctx, seed + 99, S, directed=True, n_sets=n_sets)
        smp = (p1, ni, nj, p2)
    else:
        smp = api.draw_samples(ctx, seed, S, n_sets=n_sets)
    dist = rng.uniform(0.05, 0.5, n) if diag else np.zeros(n)
    return (g["edges"], ew, g["comm"], g["embedding"], dist, vw, *EMPTY, split), smp


def _run(ctx, args, smp, directed=False, **options):
    """One sweep under `options` (restored afterwards): (7-vector, trace, stats)."""
    import cge.jl_amd as cg

    defaults = {"exact_packed": 0, "fit_persistent": 0, "bvec_blocks": 0, "pow_exp2": 1, "exact_resident_limit": 0}
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        res, tr = (cg.wGCL_directed if directed else cg.wGCL)(*args, samples=smp, trace=True, ctx=ctx)
        stats = {k: ctx.get_stat(k) for k in ("exact_packed", "exact_matrix_bytes", "fit_persistent_alphas", "fit_iterations")}
    finally:
        for k in options:
            ctx.set_option(k, defaults[k])
    return np.array(res), tr, stats


def _same_bits(a, b):
    (ra, ta, sa), (rb, tb, sb) = a, b
    assert np.array_equal(ra, rb), (ra, rb)
    assert ta["iters"] == tb["iters"] and sa["fit_iterations"] == sb["fit_iterations"]
    assert np.array_equal(ta["div"], tb["div"], equal_nan=True) and np.array_equal(ta["auc"], tb["auc"], equal_nan=True)


# (N, C, d) and what else the case varies
CASES = [
    dict(n=256, C=2, d=4),
    dict(n=257, C=5, d=9, weighted=True),
    dict(n=321, C=12, d=16, split=True),
    dict(n=700, C=30, d=2, n_sets=40),
    dict(n=1000, C=40, d=16, diag=True),  # through cg.wGCL with a non-zero `distances` vector: a positive random diagonal
]


def _packed_bound(n):
    Np = 64 * ((n + 63) // 64)
    return 4.125 * Np * Np + 256 * Np  # the tile buffer NT x 32768 plus fp_P = Np^2 / 8, exactly


@pytest.mark.parametrize("case", range(len(CASES)))
def test_packed_sweep_against_the_oracle(ctx, orc, case):
    kw = CASES[case]
    args, smp = _inputs(ctx, seed=500 + case, **kw)
    res, tr, st = _run(ctx, args, smp, exact_packed=1)
    assert st["exact_packed"] == 1 and st["fit_persistent_alphas"] == 0
    assert st["exact_matrix_bytes"] <= _packed_bound(kw["n"])
    exp, etr = orc.wGCL(*args, smp, trace=True)
    _cmp_result(res, exp, tr, etr)


@pytest.mark.parametrize("pow_exp2", [1, 0])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_packed_sweep_has_the_resident_forms_bits(ctx, case, pow_exp2):
    """With fit_persistent = 1 and bvec_blocks = 1 the resident form runs the same tile kernels in the same order: a difference
    is a defect of the packed path, not a rounding matter."""
    args, smp = _inputs(ctx, seed=500 + case, **CASES[case])
    opts = dict(fit_persistent=1, bvec_blocks=1, pow_exp2=pow_exp2)
    resident = _run(ctx, args, smp, exact_packed=0, **opts)
    packed = _run(ctx, args, smp, exact_packed=1, **opts)
    assert resident[2]["exact_packed"] == 0 and packed[2]["exact_packed"] == 1
    _same_bits(resident, packed)


def test_footprint(ctx):
    n = 1000
    args, smp = _inputs(ctx, n, 40, 16, seed=504, diag=True)
    _, _, packed = _run(ctx, args, smp, exact_packed=1)
    _, _, resident = _run(ctx, args, smp)
    assert packed["exact_packed"] == 1 and 0 < packed["exact_matrix_bytes"] <= _packed_bound(n)
    assert resident["exact_packed"] == 0 and resident["exact_matrix_bytes"] >= 16 * n * n


def test_auto_rule_and_refusal(ctx):
    """Option 0 takes the packed form exactly where the resident one would be refused (the guard's limit through the test
    knob); a directed sweep beyond the limit is still refused, and the context goes on scoring."""
    from cge.jl_amd import api

    n = 600
    args, smp = _inputs(ctx, n, 20, 8, seed=601)
    resident = _run(ctx, args, smp)
    forced = _run(ctx, args, smp, exact_packed=1)
    auto = _run(ctx, args, smp, exact_packed=0, exact_resident_limit=1_000_000)
    assert resident[2]["exact_packed"] == 0 and forced[2]["exact_packed"] == 1 and auto[2]["exact_packed"] == 1
    _same_bits(auto, forced)
    dargs, dsmp = _inputs(ctx, n, 20, 8, seed=602, directed=True)
    with pytest.raises(api.CGEError) as e:
        _run(ctx, dargs, dsmp, directed=True, exact_resident_limit=1_000_000)
    assert e.value.code == CGE_E_OOM
    args2, smp2 = _inputs(ctx, n, 20, 8, seed=601)  # (the resident graph is the undirected one again)
    again = _run(ctx, args2, smp2)  # knob back to 0
    assert again[2]["exact_packed"] == 0
    _same_bits(again, resident)


@pytest.mark.parametrize("n,C,directed", [(200, 6, False), (300, 1, False), (400, 10, True)])
def test_where_the_form_does_not_apply(ctx, n, C, directed):
    """Below 256 vertices, with one community, directed: the option changes nothing."""
    args, smp = _inputs(ctx, n, C, 6, seed=700 + n, directed=directed)
    default = _run(ctx, args, smp, directed=directed)
    asked = _run(ctx, args, smp, directed=directed, exact_packed=1)
    assert default[2]["exact_packed"] == 0 and asked[2]["exact_packed"] == 0
    _same_bits(default, asked)


def test_stale_resident_buffers_are_released(ctx):
    """A resident sweep at N = 900, then a packed one at N = 1000 on the same context: the stat counts what the sweep required,
    and the result is a fresh context's."""
    from cge.jl_amd import api

    a900, s900 = _inputs(ctx, 900, 25, 8, seed=801)
    assert _run(ctx, a900, s900)[2]["exact_packed"] == 0
    a1000, s1000 = _inputs(ctx, 1000, 40, 16, seed=802)
    packed = _run(ctx, a1000, s1000, exact_packed=1)
    assert packed[2]["exact_packed"] == 1 and packed[2]["exact_matrix_bytes"] <= _packed_bound(1000)
    fresh = api.Context(0)
    try:
        b1000, t1000 = _inputs(fresh, 1000, 40, 16, seed=802)
        assert all(np.array_equal(x, y) for x, y in zip(s1000, t1000))
        _same_bits(packed, _run(fresh, b1000, t1000, exact_packed=1))
    finally:
        fresh.close()
