"""The two forms of the bf16-split bound pass of the pruned diameter, and the reference points' distance matrix (run with
-m gpu on an MI355X).

F1  bits: the streaming form (testing knob test_pcent_form = 1) and the register-resident form (2) run the same MFMA chain per
    entry, so the bound matrix P of cge_diameter_bounds_test is equal byte for byte -- over every k-step count, partly filled,
    exact and two column super-tiles, row tiles of one to eight landmarks, overflowing accumulators and the fitness verdict;
F2  rigour on the register form itself: P >= the long double maximum (the reference of test_gpu_diameter.py, imported);
F3  rd2: the hook's distance matrix has the bits of the sequential sum of squared differences of the centred values;
F4  one score under either form: the same 7-vector and the same diameter record.

The hook runs the bound pass as ONE share (part 0 of 1): that is the part / nparts call of every case here.
"""
import numpy as np
import pytest

import test_gpu_diameter as tgd

pytestmark = pytest.mark.gpu

WIDTHS = [1, 17, 32, 33, 64, 96, 100, 128]       # KP = 32, 32, 32, 64, 64, 96, 128, 128: all four k-step counts
COMMS = [32, 129, 384, 500, 512, 513, 700]       # a partly filled 512-wide super-tile, an exact one, the step to two
CYCLE = [1, 15, 16, 17, 127, 128, 129, 300]      # landmark sizes: a 128-row tile of one to eight landmarks, a landmark over three
KINDS = ["offset", "big70", "tiny", "huge"]      # beside the Gaussian clusters every case runs


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.set_option("test_pcent_form", 0)
    c.close()


def _assignment(C, rng):
    """N = C + 8 landmarks whose sizes go round CYCLE; every community has a landmark."""
    N = C + 8
    sizes = np.array([CYCLE[a % 8] for a in range(N)])
    n = int(sizes.sum())
    v2l = np.empty(n, dtype=np.int64)
    v2l[rng.permutation(n)] = np.repeat(np.arange(1, N + 1), sizes)
    return v2l, N, np.arange(N) % C + 1


def _data(kind, rng, v2l, lcomm, d):
    """Gaussian clusters around one centre per community, then the class's change.  Returns (embedding, pass expected to run)."""
    n = len(v2l)
    centres = 5.0 * rng.standard_normal((int(lcomm.max()), d))
    X = centres[lcomm[v2l - 1] - 1] + rng.standard_normal((n, d))
    ran = 2
    if kind == "offset":
        X += 1e3
    elif kind == "big70":  # products near 2^140 overflow the fp32 accumulators: the 1e300 branch
        X *= 2.0 ** 70
    elif kind == "tiny":  # no centred value reaches 2^-40: the fp64 pass
        X *= 2.0 ** -50
        ran = 0
    elif kind == "huge":  # one centred value beyond 2^100: the fp64 pass
        X[n // 3, d // 2] = 2.0 ** 101
        ran = 0
    return np.asfortranarray(X), ran


def _forms(ctx, v2l, N, lcomm, C, what):
    out = {}
    for form in (1, 2):
        ctx.set_option("test_pcent_form", form)
        out[form] = ctx.diameter_bounds_test(v2l, N, lcomm, C, 2)
    again = ctx.diameter_bounds_test(v2l, N, lcomm, C, 2)  # a second call of the register form (buffers reused)
    ctx.set_option("test_pcent_form", 0)
    (P1, ran1, _, _), (P2, ran2, _, _) = out[1], out[2]
    assert P1.shape == (N, C) and P1.tobytes() == P2.tobytes(), (what, int((P1 != P2).sum()), np.argwhere(P1 != P2)[:3].tolist())
    assert again[0].tobytes() == P2.tobytes() and again[1] == ran2, what
    assert np.isfinite(P1).all() and (P1 >= 0).all(), what
    return P1, ran1, ran2


@pytest.mark.parametrize("C", COMMS)
@pytest.mark.parametrize("d", WIDTHS)
def test_bound_matrix_has_the_streaming_forms_bits(ctx, d, C):
    """P under test_pcent_form 1 and 2 is byte-equal, pass_ran == 2 both times; the unfit classes report the fp64 pass under
    either knob.  Every (d, C) runs the Gaussian clusters and one further class, which goes round with (d, C)."""
    rng = np.random.default_rng(100 * d + C)
    v2l, N, lcomm = _assignment(C, rng)
    for kind in ("clusters", KINDS[(WIDTHS.index(d) + COMMS.index(C)) % len(KINDS)]):
        emb, expect = _data(kind, rng, v2l, lcomm, d)
        tgd._load(ctx, emb)
        P, ran1, ran2 = _forms(ctx, v2l, N, lcomm, C, (d, C, kind))
        assert ran1 == expect and ran2 == expect, (d, C, kind, ran1, ran2)
        if kind == "big70":
            assert (P == 1e300).any(), (d, C, "no accumulator overflowed: the 1e300 branch was not taken")


@pytest.mark.parametrize("d,C", [(17, 129), (64, 32), (96, 129), (128, 129)])
def test_register_form_dominates_the_long_double_maximum(ctx, d, C):
    """The register-resident form on its own: every entry of P >= the long double maximum, and no looser than the pass's margin.
    (One shape per k-step count, at the widths where n C d long double operations take a second.)"""
    rng = np.random.default_rng(7 * d + C)
    v2l, N, lcomm = _assignment(C, rng)
    emb, _ = _data("clusters", rng, v2l, lcomm, d)
    tgd._load(ctx, emb)
    ctx.set_option("test_pcent_form", 2)
    try:
        _, ran = tgd._check_bounds(ctx, emb, v2l, N, lcomm, C, 2, {}, (d, C))
    finally:
        ctx.set_option("test_pcent_form", 0)
    assert ran == 2


@pytest.mark.parametrize("d", [1, 16, 17, 128])
@pytest.mark.parametrize("nref", [1, 31, 32, 33, 500, 513])
def test_reference_distances_are_the_sequential_sums(ctx, nref, d):
    """rd2[a][b] = the sum over k ascending of (fl(a_k - m_k) - fl(b_k - m_k))^2, every operation rounded once: equal bytes,
    symmetric to the bit, zero diagonal."""
    rng = np.random.default_rng(1000 * nref + d)
    tgd._load(ctx, np.asfortranarray(3.0 + rng.standard_normal((64, d))))
    refs = 3.0 + 2.0 * rng.standard_normal((nref, d))
    rd2, mean = ctx.ref_dist2_test(refs)
    xc = refs - mean
    exp = np.zeros((nref, nref))
    for k in range(d):
        df = xc[:, k][:, None] - xc[:, k][None, :]
        exp = exp + df * df
    assert rd2.tobytes() == exp.tobytes(), (nref, d, int((rd2 != exp).sum()))
    assert rd2.tobytes() == rd2.T.copy().tobytes() and not rd2.diagonal().any(), (nref, d)


def test_one_score_is_the_same_under_either_form(ctx):
    """n = 20 000, 400 communities, 1 200 landmarks, d = 64: the 7-vector and the diameter record under the knob at 1 and 2."""
    from cge.jl_amd import synth

    g = synth.abcd_like(20000, 200000, 400, 64, seed=11)
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
    got = {}
    try:
        ctx.set_option("diameter", 2)  # the pruned search, so that the bound pass runs
        for form in (1, 2):
            ctx.set_option("test_pcent_form", form)
            res = ctx.score(g["clusters"], 1200, 4, "rss", seed=3, auc_samples=2000)
            assert ctx.get_stat("diameter_bound_pass") == 2, form
            got[form] = (res, ctx.last_diameter())
    finally:
        ctx.set_option("test_pcent_form", 0)
        ctx.set_option("diameter", 0)
    assert got[1][0].tobytes() == got[2][0].tobytes(), (got[1][0].tolist(), got[2][0].tolist())
    assert got[1][1] == got[2][1] and got[1][1][1] == "pruned", (got[1][1], got[2][1])
