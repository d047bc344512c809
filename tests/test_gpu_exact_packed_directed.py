"""Whole directed exact sweeps in the packed form (option "exact_packed_directed": the upper tiles of the current alpha's GD and
two sets of partial vectors are the only O(N^2) device storage): against the oracle, against the resident tile form bit for bit,
the footprint, the auto rule and the refusal it replaces, the shapes the form does not apply to, and buffers across sweeps on one
context.  It mirrors tests/test_gpu_exact_packed.py, whose undirected sweeps the option must leave alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's tolerance against the oracle (tests/test_gpu_parity.py)
EMPTY = ([], [], np.zeros((0, 2), np.int64), [], np.zeros((0, 0)))
CGE_E_OOM = -6
DEFAULTS = {"exact_packed": 0, "exact_packed_directed": 0, "fit_persistent": 0, "bvec_blocks": 0, "pow_exp2": 1,
            "exact_resident_limit": 0, "fit_dir_tiles": 0}


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


def _inputs(ctx, n, C, d, seed, weighted=False, split=False, n_sets=1, diag=False, directed=True, S=800):
    """A synthetic graph, its samples (drawn once, handed to both sides; directed: with the second positive draw) and the wGCL
    argument tuple -- tests/test_gpu_exact_packed.py::_inputs."""
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


def _run(ctx, args, smp, directed=True, **options):
    """One sweep under `options` (restored afterwards): (7-vector, trace, stats)."""
    import cge.jl_amd as cg

    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        res, tr = (cg.wGCL_directed if directed else cg.wGCL)(*args, samples=smp, trace=True, ctx=ctx)
        stats = {k: ctx.get_stat(k) for k in ("exact_packed", "exact_matrix_bytes", "fit_persistent_alphas", "fit_iterations")}
    finally:
        for k in options:
            ctx.set_option(k, DEFAULTS[k])
    return np.array(res), tr, stats


def _same_bits(a, b):
    (ra, ta, sa), (rb, tb, sb) = a, b
    assert np.array_equal(ra, rb), (ra, rb)
    assert ta["iters"] == tb["iters"] and sa["fit_iterations"] == sb["fit_iterations"]
    assert np.array_equal(ta["div"], tb["div"], equal_nan=True) and np.array_equal(ta["auc"], tb["auc"], equal_nan=True)


# (N, C, d) and what else the case varies; case k is drawn with seed 900 + k
CASES = [
    dict(n=256, C=2, d=4),
    dict(n=257, C=5, d=9, weighted=True),
    dict(n=321, C=12, d=16, split=True),
    dict(n=700, C=30, d=2, n_sets=40),
    dict(n=1000, C=40, d=16, diag=True),  # a positive random `distances` diagonal
]


def _packed_bound(n):
    Np = 64 * ((n + 63) // 64)
    return 4.25 * Np * Np + 256 * Np  # the tile buffer NT x 32768 plus two sets of partial vectors of Np^2 / 8 bytes, exactly


@pytest.mark.parametrize("case", range(len(CASES)))
def test_packed_directed_sweep_against_the_oracle(ctx, orc, case):
    kw = CASES[case]
    args, smp = _inputs(ctx, seed=900 + case, **kw)
    res, tr, st = _run(ctx, args, smp, exact_packed_directed=2)
    assert st["exact_packed"] == 1 and st["fit_persistent_alphas"] == 0
    assert 0 < st["exact_matrix_bytes"] <= _packed_bound(kw["n"])
    exp, etr = orc.wGCL_directed(*args, smp, trace=True)
    _cmp_result(res, exp, tr, etr)


@pytest.mark.parametrize("pow_exp2", [1, 0])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_packed_directed_sweep_has_the_resident_tile_forms_bits(ctx, case, pow_exp2):
    """With fit_persistent = 1, bvec_blocks = 1 and the testing option fit_dir_tiles = 1 the resident form runs the same tile
    kernels on a row-major matrix, in the same order: a difference is a defect of the packed path, not a rounding matter."""
    args, smp = _inputs(ctx, seed=900 + case, **CASES[case])
    opts = dict(fit_persistent=1, bvec_blocks=1, fit_dir_tiles=1, pow_exp2=pow_exp2)
    resident = _run(ctx, args, smp, exact_packed_directed=0, **opts)
    packed = _run(ctx, args, smp, exact_packed_directed=2, **opts)
    assert resident[2]["exact_packed"] == 0 and packed[2]["exact_packed"] == 1
    _same_bits(resident, packed)


def test_auto_rule_and_refusal(ctx):
    """Option 1 takes the packed form exactly where the resident one would be refused (the guard's limit through the test knob);
    option 0 is refused there with a message that names the option, and the context goes on scoring."""
    from cge.jl_amd import api

    n = 600
    args, smp = _inputs(ctx, n, 20, 8, seed=911)
    default = _run(ctx, args, smp)
    forced = _run(ctx, args, smp, exact_packed_directed=2)
    auto = _run(ctx, args, smp, exact_packed_directed=1, exact_resident_limit=1_000_000)
    assert default[2]["exact_packed"] == 0 and forced[2]["exact_packed"] == 1 and auto[2]["exact_packed"] == 1
    _same_bits(auto, forced)
    with pytest.raises(api.CGEError) as e:
        _run(ctx, args, smp, exact_packed_directed=0, exact_resident_limit=1_000_000)
    assert e.value.code == CGE_E_OOM and "exact_packed_directed" in str(e.value), str(e.value)
    again = _run(ctx, args, smp)  # knob back to 0: the context scores on
    assert again[2]["exact_packed"] == 0
    _same_bits(again, default)
    unlimited = _run(ctx, args, smp, exact_packed_directed=1)  # option 1 without the knob: resident, the default's bits
    assert unlimited[2]["exact_packed"] == 0
    _same_bits(unlimited, default)


@pytest.mark.parametrize("n,C", [(200, 6), (300, 1)])
def test_where_the_form_does_not_apply(ctx, n, C):
    """Below 256 vertices, with one community: option 2 changes nothing."""
    args, smp = _inputs(ctx, n, C, 6, seed=920 + n)
    default = _run(ctx, args, smp)
    asked = _run(ctx, args, smp, exact_packed_directed=2)
    assert default[2]["exact_packed"] == 0 and asked[2]["exact_packed"] == 0
    _same_bits(default, asked)
    assert default[2]["exact_matrix_bytes"] == asked[2]["exact_matrix_bytes"]


@pytest.mark.parametrize("exact_packed", [0, 1])
def test_undirected_sweeps_do_not_see_the_option(ctx, exact_packed):
    args, smp = _inputs(ctx, 321, 12, 16, seed=930, directed=False)
    without = _run(ctx, args, smp, directed=False, exact_packed=exact_packed, exact_packed_directed=0)
    with_it = _run(ctx, args, smp, directed=False, exact_packed=exact_packed, exact_packed_directed=2)
    assert without[2] == with_it[2] and without[2]["exact_packed"] == exact_packed
    _same_bits(without, with_it)


def _fresh(n, C, d, seed, samples, directed, **options):
    from cge.jl_amd import api

    fresh = api.Context(0)
    try:
        args, smp = _inputs(fresh, n, C, d, seed=seed, directed=directed)
        assert all(np.array_equal(x, y) for x, y in zip(samples, smp))
        return _run(fresh, args, smp, directed=directed, **options)
    finally:
        fresh.close()


def test_buffers_across_sweeps_on_one_context(ctx):
    """Directed resident at n = 900, then directed packed at n = 1000; then undirected packed at n = 700 (whose partial vectors are
    half the directed ones): each result is a fresh context's, and the stat counts what the sweep required."""
    a900, s900 = _inputs(ctx, 900, 25, 8, seed=941)
    assert _run(ctx, a900, s900)[2]["exact_packed"] == 0
    a1000, s1000 = _inputs(ctx, 1000, 40, 16, seed=942)
    packed = _run(ctx, a1000, s1000, exact_packed_directed=2)
    assert packed[2]["exact_packed"] == 1 and packed[2]["exact_matrix_bytes"] <= _packed_bound(1000)
    _same_bits(packed, _fresh(1000, 40, 16, 942, s1000, True, exact_packed_directed=2))
    a700, s700 = _inputs(ctx, 700, 30, 2, seed=943, directed=False)
    und = _run(ctx, a700, s700, directed=False, exact_packed=1)
    assert und[2]["exact_packed"] == 1
    ref = _fresh(700, 30, 2, 943, s700, False, exact_packed=1)
    _same_bits(und, ref)
    assert und[2]["exact_matrix_bytes"] == ref[2]["exact_matrix_bytes"]
