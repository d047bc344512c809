"""The vect_B half of the fused fit's epilogue (csrc/fit_flow_body.inc) tile partial by tile partial and bin by bin, beside the
tallies that share its launch (run with -m gpu on an MI355X).

Everything goes through the testing hook cge_fused_chain_test: one alpha of an undirected landmark-mode sweep on a caller's
problem -- the layout and its tables, the epilogue's table, fit_flow_kernel<.., FUSED = true> (one problem) or
fit_flow_multi_kernel (several) with the epilogue's outputs wanted, the bins and the divergence -- by the sweep's own functions.
The references are tests/fused_chain_ref.py (np.longdouble, pinned on the CPU by tests/test_fused_chain_ref.py), always on the
device's own power matrix (cge_fit_test form 1, want_GD) and the iterate the hook returned, so the power's and the fit's own
errors stay out.  The shapes are fused_chain_ref.sizes(): community sizes in id order, the vertex order shuffled; which geometry
a size sits on is derived from the device's CU count.

F1  no tile partial is NaN after a converged launch; every one within (n_terms + 3) 2^-53 ref of the long double value (all terms
    non-negative: two roundings per product, at most n - 1 additions, one unit for the reference) and exactly 0.0 without terms;
F2  every bin of vect_B within the same bound, the guard behind it still NaN; vect_B and js_fused bit for bit what
    cge_vect_b_test form 5 gives on the same GD and T; js_fused within 1e-12 of the long double JS; n_modes 1 and 2;
F3  the final iterate: delta = 1e300 (the first check ends the fit), a delta of several iterations, a start skew of 20 naps --
    T and iters those of cge_fit_test form 4 on the problem in the layout's order, F1 and F2 on the returned T;
F4  an abandoned launch: status 1, every partial and tally still NaN;
F5  the tallies beside vect_B on synthetic operands (S = 1, 255, 256, 257, 16389): part and apw bit for bit the reference's,
    want = 3 gives want = 1's partials / vect_B / T / iters and want = 2's part;
F6  every refusal by its message; the context scores as before afterwards;
F7  members of one fit_flow_multi_kernel launch equal their own single launches bit for bit.

Measured on an MI355X (256 CUs; `-s` prints the figures): the largest device error as a fraction of its tolerance, over all
shapes and alphas, is 0.35 for F1 (the tile partials) and 0.335 for F2 (the bins).

What the tests found: the epilogue wrote no partial for an id without a member inside a block's range of ids (640x10e: the two
empty ids between a community of 60 and one of 96), where bvec_tile_kernel writes +0.0; nothing reads those partials, but F1's
"no NaN" spoke.  The epilogue now writes +0.0 there, on a path that tiles without empty ids never take.

Scratch mutants of the epilogue (not committed) and what noticed them:
  stage (a) treating a chunk's first column as continuing the previous chunk's piece (pm = segJ) -- F1's NaN check and bound at
    every shape and alpha, and with it F2, F3, F7; not F5, which compares the epilogue with itself;
  `dead` with >= instead of > (the diagonal dropped) -- F1's bound on the partials of every diagonal tile, at every shape and
    alpha, F2, F3; not F5 / F7, which compare the epilogue with itself;
  stage (c) without the write of the last row run -- F1's NaN check at every shape, F2, F3, F4's second run, F7, and the score of
    F6 (NaN);
  ehdr[..][6] = ns[I] instead of ns[J] -- F1's NaN check at every shape with a tile whose blocks span different numbers of ids
    (all but 256x2 and 513x8), F2, F3, F5, F7 and the score of F6 (run with the partials' buffer enlarged, since the mutant
    writes past a tile's slots);
  kfin = k for a wave that left on its own -- nothing, and nothing can: Tf, the one use of kfin, is read by the tallies alone,
    which only workgroups with a quarter block run (kfin = k there already); vect_B's T of such a wave is what it staged for its
    last products (tsh), which F1 / F3 hold to the fit's T at 1985x40, where 4 of the 132 workgroups have no quarter block.
"""
import functools

import numpy as np
import pytest

import fit_ref as fr
import fused_chain_ref as fc

pytestmark = pytest.mark.gpu

LD = fc.LD
U = fc.U
E_ARG = -7
SMALL = ["256x2", "257x5", "321x3", "513x8", "700x17", "640x10e", "pieces32"]
ALPHAS = [0.25, 3.0, 10.0]
BIG_ALPHA = 3.0


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


def _geo(N):
    g = fc.geometry(N, _cus())
    return g if g and g["NSB"] == 1 else None


def _needs(name):
    """Skip a big shape whose purpose this device's CU count does not give."""
    N = sum(fc.sizes(name))
    g = _geo(N)
    if name == "1985x40" and not (g and g["G"] > 4 * g["Nt"]):
        pytest.skip("no workgroup without a quarter block at N = 1985 on %d CUs" % _cus())
    if name == "2817x50" and not (g and g["NW"] == 8):
        pytest.skip("N = 2817 is not on the 8-wave fused instance on %d CUs" % _cus())
    assert g, name


def test_the_sizes_reach_what_they_are_chosen_for():
    if _cus() != 256:
        return  # (the table of fused_chain_ref.sizes is that of 256 CUs; every other test derives its geometry from the CU count)
    g = {n: _geo(sum(fc.sizes(n))) for n in SMALL + ["1985x40", "2817x50"]}
    assert all(g[n] and g[n]["NW"] == 4 and g[n]["G"] == 4 * g[n]["Nt"] for n in SMALL)
    assert g["1985x40"]["G"] == 132 > 4 * 32 and g["2817x50"]["NW"] == 8


# ---- the problems --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _base(name):
    """comm, C, D (random symmetric in [0, 1], zero diagonal, one entry exactly 1 and one off-diagonal entry exactly 0), vC."""
    seed = sum(map(ord, name))
    comm, C = fc.shuffled_comm(name, seed)
    N = comm.size
    rng = np.random.default_rng(seed + 7)
    D = rng.random((N, N))
    D = np.triu(D, 1)
    D[3, N - 2] = 1.0  # GD = 0
    D[1, N // 2] = 0.0  # GD = 1
    D = D + D.T
    assert np.array_equal(D, D.T) and D.max() == 1.0 and D.min() == 0.0
    vC = np.floor(rng.random(C * (C + 1) // 2) * 60.0 - 6.0).clip(0.0)
    return comm, C, D, vC, rng.normal(size=N), rng.uniform(-1.0, 1.0, size=N)


@functools.lru_cache(maxsize=4)
def _problem(name, alpha):
    comm, C, D, vC, z, u = _base(name)
    GD = (1.0 - D) ** alpha
    Th = np.exp(0.5 * z)
    w = Th * (GD @ Th) * (1.0 + 0.3 * u)
    return {"D": D, "alpha": float(alpha), "w": w, "T0": np.ones(comm.size), "comm": comm, "C": C, "vC": vC}


_gd_cache = {}


def _device_gd(ctx, name, alpha):
    """The symmetric power matrix as the device makes it (k_pow_matrix under pow_exp2 shares log_parts / exp2_parts with the fused
    prologue; tests/test_gpu_fit.py holds form 4 to form 3)."""
    if (name, alpha) not in _gd_cache:
        _gd_cache.clear()
        ran, (out,) = ctx.fit_test(_problem(name, alpha), form=1, delta=1e300, want_GD=True)
        assert ran == 1 and out["iters"] == 1
        GD = fr.symmetric(out["GD"])
        assert GD.min() == 0.0 and GD.max() == 1.0 and not np.any(np.isnan(GD))
        _gd_cache[(name, alpha)] = GD
    return _gd_cache[(name, alpha)]


def _delta(pr, several=True):
    """`several`: a threshold a few orders below the first change, which the fit reaches after several iterations."""
    return 1e-3 * float(np.max(pr["w"])) if several else 1e300


def _chain(ctx, pr, delta, want=1, n_modes=1, tally=None):
    (out,) = ctx.fused_chain_test(dict(pr, want=want, n_modes=n_modes, tally=tally), delta=delta)
    return out


def _form4(ctx, pr, order, delta):
    """cge_fit_test form 4 on the same problem as the hook's launch saw it: in the layout's order (a row's additions follow the
    numbering, so the caller's order would give other bits).  T comes back in the caller's numbering."""
    o = np.asarray(order, dtype=np.int64)
    ran, (f4,) = ctx.fit_test({"D": pr["D"][np.ix_(o, o)], "alpha": pr["alpha"], "w": pr["w"][o], "T0": pr["T0"][o]}, form=4, delta=delta)
    assert ran == 4 and f4["status"] == 0
    T = np.empty_like(f4["T"])
    T[o] = f4["T"]
    return f4["iters"], T


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    print(f"  {key}: largest error / tolerance so far {_worst[key]:.3g}")


def _within(got, ref, nk, key, what):
    err = np.abs(LD(got) - ref)
    bound = (LD(nk) + 3) * U * ref
    bad = np.flatnonzero(~(err <= bound))  # (~: a NaN fails)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], ref[bad[:8]], nk[bad[:8]])
    empty = nk == 0
    assert np.all(got[empty] == 0.0) and not np.any(np.signbit(got[empty])), what
    live = ~empty & (ref > 0)
    if live.any():
        _note(key, np.max(err[live] / bound[live]))


# ---- JS in long double, straight from src/auxilary.jl:34-52 ---------------------------------------------------------------------
def _js_ref(vC, vB, sel):
    n = int(sel.sum())
    if n == 0:
        return LD(0)
    c, b = LD(vC[sel]), LD(vB[sel])
    p, q = (c + 1) / (c.sum() + n), (b + 1) / (b.sum() + n)
    m = (p + q) / 2
    return (np.sum(p * np.log(p / m)) + np.sum(q * np.log(q / m))) / 2


def _check_js(js_fused, vC, vB, C, n_modes, what):
    i = np.arange(C, dtype=np.int64)
    vI = np.zeros(vC.size, bool)
    vI[C * i - i * (i - 1) // 2] = True  # idx(C, i, i) - 1
    sels = [np.ones(vC.size, bool)] if n_modes == 1 else [vI, ~vI]
    assert js_fused.shape == (n_modes,)
    for got, sel in zip(js_fused, sels):
        ref = float(_js_ref(vC, vB, sel))
        if int(sel.sum()) <= 1:  # one bin (p = q = m = 1): exactly zero in the reference, and on the device
            assert ref == 0.0 and got == 0.0, (what, got)
        else:  # (V4 of tests/test_gpu_vect_b.py) the relative tolerance means something only away from cancellation
            assert ref >= 1e-3, (what, ref)
            assert got == pytest.approx(ref, rel=1e-12), what


def _check_tables(out, lay, what):
    assert np.array_equal(out["order"], lay["order"]), what
    assert np.array_equal(out["fc"], lay["fc"]) and np.array_equal(out["ns"], lay["ns"]), what
    assert np.array_equal(out["base"], lay["base"]) and out["bt_total"] == lay["bt_total"] == out["partials"].size, what


def _check_f1_f2(ctx, name, alpha, pr, out, n_modes, what, against_form5=True):
    """F1 and F2 of one converged launch on the T it returned."""
    GD = _device_gd(ctx, name, alpha)
    comm, C, T = pr["comm"], pr["C"], out["T"]
    assert out["status"] == 0 and not np.any(np.isnan(T)), what
    lay = fc.layout(comm, C)
    _check_tables(out, lay, what)
    assert not np.any(np.isnan(out["partials"])), (what, np.flatnonzero(np.isnan(out["partials"]))[:8])
    ref, cnt = fc.partials(GD, T, lay)
    _within(out["partials"], ref, cnt, "F1", (what, "partials"))
    bref, nk = fc.vect_b(GD, T, comm, C)
    assert np.all(np.isnan(out["guard"])), (what, "written past the vector's end")
    _within(out["vectB"], bref, nk, "F2", (what, "vectB"))
    _check_js(out["js_fused"], pr["vC"], out["vectB"], C, n_modes, what)
    if against_form5:
        r = ctx.vect_b_test(GD, T, T, comm, C, form=5, vC=pr["vC"], n_modes=n_modes)
        assert r["form_ran"] == 5
        assert _same_bits(out["vectB"], r["vectB"]), (what, np.flatnonzero(out["vectB"] != r["vectB"])[:8])
        assert _same_bits(out["js_fused"], r["js_fused"]), (what, out["js_fused"], r["js_fused"])


# ---- F1, F2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", SMALL)
def test_partials_and_bins_against_the_definition(ctx, name, alpha):
    pr = _problem(name, alpha)
    outs = {}
    for n_modes in (1, 2):
        outs[n_modes] = out = _chain(ctx, pr, _delta(pr), n_modes=n_modes)
        assert out["iters"] >= 3, out["iters"]
        _check_f1_f2(ctx, name, alpha, pr, out, n_modes, (name, alpha, n_modes))
    assert _same_bits(outs[1]["partials"], outs[2]["partials"]) and _same_bits(outs[1]["vectB"], outs[2]["vectB"])
    assert _same_bits(outs[1]["T"], outs[2]["T"])


@pytest.mark.parametrize("name", ["1985x40", "2817x50"])
def test_partials_and_bins_on_the_big_geometries(ctx, name):
    """1985 (on 256 CUs): tile waves in workgroups without a quarter block, which leave by the end mark on their own; 2817: the
    8-wave instance.  Once each, n_modes = 2."""
    _needs(name)
    pr = _problem(name, BIG_ALPHA)
    out = _chain(ctx, pr, _delta(pr), n_modes=2)
    assert out["iters"] >= 3
    iters4, T4 = _form4(ctx, pr, out["order"], _delta(pr))
    assert iters4 == out["iters"] and _same_bits(T4, out["T"])
    _check_f1_f2(ctx, name, BIG_ALPHA, pr, out, 2, name)


# ---- F3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["256x2", "700x17", "1985x40"])
def test_the_final_iterate_is_the_fit_s(ctx, name):
    if name == "1985x40":
        _needs(name)
    alpha = BIG_ALPHA
    pr = _problem(name, alpha)
    cases = [("first check", 1e300)] + ([("several", _delta(pr))] if name != "1985x40" else [])  # (1985 several: the test above)
    for what, delta in cases:
        out = _chain(ctx, pr, delta, n_modes=1)
        iters4, T4 = _form4(ctx, pr, out["order"], delta)
        assert out["iters"] == iters4 and _same_bits(out["T"], T4), (name, what, out["iters"], iters4)
        assert (out["iters"] == 1) == (delta == 1e300)
        _check_f1_f2(ctx, name, alpha, pr, out, 1, (name, what), against_form5=name != "1985x40")
        try:  # a start skew must not change a bit
            ctx.set_option("fit_persistent_test_delay", 20)
            late = _chain(ctx, pr, delta, n_modes=1)
        finally:
            ctx.set_option("fit_persistent_test_delay", 0)
        assert late["iters"] == out["iters"] and late["status"] == 0
        for k in ("T", "partials", "vectB", "js_fused"):
            assert _same_bits(late[k], out[k]), (name, what, k)


# ---- F4 ----------------------------------------------------------------------------------------------------------------------
def test_an_abandoned_launch_writes_nothing(ctx):
    pr = _problem("257x5", 3.0)
    tally = fc.tally_inputs(257, 257, 11)
    try:
        ctx.set_option("fit_persistent_test_timeout", 1)
        out = _chain(ctx, pr, _delta(pr), want=3, tally=tally)
    finally:
        ctx.set_option("fit_persistent_test_timeout", 0)
    assert out["status"] == 1
    assert out["bt_total"] > 0 and np.all(np.isnan(out["partials"])) and np.all(np.isnan(out["part"]))
    assert np.all(np.isnan(out["T"])) and np.all(np.isnan(out["vectB"])) and np.all(np.isnan(out["guard"]))
    again = _chain(ctx, pr, _delta(pr), want=3, tally=tally)  # and back
    assert again["status"] == 0 and not np.any(np.isnan(again["partials"])) and not np.any(np.isnan(again["part"]))


# ---- F5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["257x5", "700x17", "1985x40"])
def test_the_tallies_share_the_launch(ctx, name):
    if name == "1985x40":
        _needs(name)
    alpha = BIG_ALPHA
    pr = _problem(name, alpha)
    N = pr["comm"].size
    delta = _delta(pr)
    one = _chain(ctx, pr, delta, want=1)
    for S in (1, 255, 256, 257, 16389):  # (16389 > 64 * 256: the block stride wraps)
        t = fc.tally_inputs(N, S, 1000 * N + S)
        ppos, pneg = ctx.pow_test(t["dpos"], alpha, 0), ctx.pow_test(t["dneg"], alpha, 0)
        two = _chain(ctx, pr, delta, want=2, tally=t)
        assert two["status"] == 0 and two["iters"] == one["iters"] and _same_bits(two["T"], one["T"])
        assert np.all(np.isnan(two["partials"])) and np.all(np.isnan(two["vectB"]))  # not wanted: not written
        gap = fc.min_tally_gap(two["T"], t["aidx"], t["afac"], ppos, pneg)
        assert gap > 1e-6, (name, S, gap)  # (the inputs' precondition, on the device's own T and powers)
        ref = fc.tallies(two["T"], t["aidx"], t["afac"], t["aden"], t["wts"], ppos, pneg)
        assert _same_bits(two["part"], ref), (name, S, np.flatnonzero(two["part"] != ref)[:8])
        assert _same_bits(two["apw"], np.stack([ppos, pneg])), (name, S)
        if S in (257, 16389):
            both = _chain(ctx, pr, delta, want=3, tally=t)
            assert both["iters"] == one["iters"]
            for k in ("T", "partials", "vectB"):
                assert _same_bits(both[k], one[k]), (name, S, k)
            assert _same_bits(both["part"], two["part"]) and _same_bits(both["apw"], two["apw"]), (name, S)
            assert np.all(np.isnan(both["guard"]))


# ---- F6 ----------------------------------------------------------------------------------------------------------------------
def _refused(ctx, text, pr, **kw):
    from cge.jl_amd import api

    with pytest.raises(api.CGEError) as e:
        ctx.fused_chain_test(dict({"want": 1}, **pr) if isinstance(pr, dict) else pr, **kw)
    assert e.value.code == E_ARG and "fused_chain_test" in str(e.value) and text in str(e.value), str(e.value)


def _plain(name, comm=None, C=None):
    """A problem of a shape that is only refused: nothing of it is computed."""
    if comm is None:
        comm, C = fc.shuffled_comm(name, 1)
    N = comm.size
    return {"D": np.zeros((N, N)), "alpha": 1.0, "w": np.ones(N), "T0": np.ones(N), "comm": comm, "C": C}


def test_refusals(ctx):
    from cge.jl_amd import synth

    g = synth.abcd_like(3000, 30000, 10, 8, seed=4)
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    ctx.set_embedding(g["embedding"])
    before = ctx.score(g["clusters"], 300, seed=5, auc_samples=2000)
    small = _problem("256x2", 3.0)
    _refused(ctx, "more than 32 pieces", _plain("pieces33"))
    _refused(ctx, "more than 32 pieces", _plain("1100x600"))
    # 150 singletons on the odd ids, then 150 vertices of id 300: block 0 spans 127 ids
    _refused(ctx, "more than 64 community ids", _plain(None, comm=np.r_[np.arange(150) * 2 + 1, np.full(150, 300)], C=300))
    _refused(ctx, "256 vertices", _plain(None, comm=np.r_[np.full(128, 1), np.full(127, 2)], C=2))
    _refused(ctx, "2 communities", _plain(None, comm=np.full(256, 1), C=1))
    try:
        ctx.set_option("pow_exp2", 0)
        _refused(ctx, "pow_exp2", small)
    finally:
        ctx.set_option("pow_exp2", 1)
    N = next(n for n in range(256, 64 * 66, 64) if _geo(n + 1) is None) + 1  # the first size off the fused geometry
    _refused(ctx, "declines N = %d" % N, _plain(None, comm=np.r_[np.full(N // 2, 1), np.full(N - N // 2, 2)], C=2))
    _refused(ctx, "want = 0", dict(small, want=0))
    _refused(ctx, "undirected only", small, directed=True)
    # several problems
    _refused(ctx, "at most 16", [dict(small, want=1)] * 17)
    n4 = max(n for n in range(256, N, 64) if _geo(n) and _geo(n)["NW"] == 4)
    if _geo(n4 + 1):  # problems on 4 and on 8 waves per workgroup
        _refused(ctx, "one NW", [dict(small, want=1), dict(_plain(None, comm=np.r_[np.full(n4, 1), np.full(1, 2)], C=2), want=1)])
    mid = dict(_plain(None, comm=np.r_[np.full(350, 1), np.full(350, 2)], C=2), want=1)
    assert _cus() // _geo(700)["G"] + 1 <= 16
    _refused(ctx, "workgroups in all", [mid] * (_cus() // _geo(700)["G"] + 1))
    after = ctx.score(g["clusters"], 300, seed=5, auc_samples=2000)
    assert np.array_equal(before, after)
    out = _chain(ctx, small, _delta(small))  # and the hook runs
    assert out["status"] == 0


# ---- F7 ----------------------------------------------------------------------------------------------------------------------
def test_members_of_a_shared_launch_equal_their_single_launches(ctx):
    alpha = BIG_ALPHA
    a, b, c3 = _problem("256x2", alpha), _problem("700x17", alpha), _problem("321x3", alpha)
    tb = fc.tally_inputs(700, 257, 77)
    tc = fc.tally_inputs(321, 16389, 78)
    members = {"a": dict(a, want=1, n_modes=1, tally=None), "b": dict(b, want=3, n_modes=2, tally=tb),
               "c": dict(c3, want=2, n_modes=1, tally=tc)}
    delta = 1e-3 * min(float(np.max(m["w"])) for m in members.values())
    single = {k: ctx.fused_chain_test(m, delta=delta)[0] for k, m in members.items()}
    for group in (["a", "b"], ["c", "b", "a"]):
        geos = [_geo(members[k]["comm"].size) for k in group]
        assert len({g["NW"] for g in geos}) == 1 and sum(g["G"] for g in geos) <= _cus()
        outs = ctx.fused_chain_test([members[k] for k in group], delta=delta)
        for k, out in zip(group, outs):
            ref = single[k]
            assert out["status"] == 0 and out["iters"] == ref["iters"], (group, k, out["iters"], ref["iters"])
            for f in ("T", "partials", "vectB", "guard", "js_fused", "part") + (("apw",) if members[k]["tally"] else ()):
                assert np.array_equal(out[f], ref[f], equal_nan=True), (group, k, f)
            for f in ("order", "fc", "ns", "base"):
                assert np.array_equal(out[f], ref[f]), (group, k, f)
    assert not np.any(np.isnan(single["b"]["part"])) and not np.any(np.isnan(single["b"]["partials"]))
