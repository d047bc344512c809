"""The exact-mode tallies of a directed sweep on the packed tiles: tally form 5 of the testing hook cge_local_score_test
(k_auc_exact -> auc_exact_kernel<true>, ordered pairs through cge_packed_index) at N = 130 (3 tiles per side) equals form 2
directed on the same symmetric GD bit for bit, and the host reference of tests/local_score_ref.py.  The pairs lie on both sides of
the diagonal, inside diagonal tiles (whose lower halves are stored) and below them (where the mirrored element is the one stored)."""
import numpy as np
import pytest

import local_score_ref as ls

pytestmark = pytest.mark.gpu

N = 130


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _case(S, seed=2):
    """local_score_ref.exact_matrix_case's symmetric GD with a directed sweep's two vectors and ordered pairs: exact values, ties
    at every 16th sample."""
    c = ls.exact_matrix_case(S, N=N, seed=seed, directed=False)
    rng = np.random.default_rng(seed + 50)
    c["Tb"] = rng.choice([1.0, 1.5, 2.0, 3.0], N)
    pi, pj = ls.random_pairs(rng, S, N, True)
    ni, nj = ls.random_pairs(rng, S, N, True)
    same = np.arange(S) % 16 == 0
    ni[same], nj[same] = pi[same], pj[same]
    c["pairs"] = (pi, pj, ni, nj, ls.sample_weights(S))
    return c


@pytest.mark.parametrize("S", [1, 4096, 65536 + 300])  # one sample, the narrow grid, the wide grid and its fold
def test_form_5_is_form_2_directed_and_the_reference(ctx, S):
    c = _case(S)
    pi, pj, ni, nj, wts = c["pairs"]
    assert np.array_equal(c["GD"], c["GD"].T) and not np.array_equal(c["Ta"], c["Tb"])
    if S >= 4096:
        for a, b in ((pi, pj), (ni, nj)):  # where the pairs lie
            ta, tb = a // 64, b // 64
            assert np.any(ta > tb) and np.any(ta < tb)  # below and above the diagonal tiles
            assert np.any((ta == tb) & (a > b)) and np.any((ta == tb) & (a < b))  # both halves of a diagonal tile
            assert np.any((ta == 2) | (tb == 2))  # the ragged last tile (two rows wide)
    pos, neg = ls.values_exact(c["GD"], c["Ta"], c["Tb"], pi, pj), ls.values_exact(c["GD"], c["Ta"], c["Tb"], ni, nj)
    if S >= 4096:
        assert np.count_nonzero(pos == neg) >= S // 16 and np.any(pos > neg) and np.any(pos < neg)
    t = dict(form=2, N=N, GD=c["GD"], Ta=c["Ta"], Tb=c["Tb"])
    o2 = ctx.local_score_test(S, directed=True, pairs=c["pairs"], tally=t)
    o5 = ctx.local_score_test(S, directed=True, pairs=c["pairs"], tally=dict(t, form=5))
    assert np.array_equal(o5["part"], o2["part"]) and np.array_equal(o5["out2"], o2["out2"])
    num, den, cnt, (tn, td) = ls.tally(pos, neg, wts)
    part = o5["part"]
    bad = np.flatnonzero((part[:, 0] != num.astype(np.float64)) | (part[:, 1] != den.astype(np.float64)))
    assert bad.size == 0, (S, bad[:8], part[bad[:8]], num[bad[:8]], den[bad[:8]])
    assert o5["out2"][0] == float(tn) and o5["out2"][1] == float(td), (o5["out2"], tn, td)


def test_form_5_reads_the_upper_tiles_alone(ctx):
    """NaN everywhere below the diagonal tiles of the caller's GD: form 5 packs and reads the upper tiles, so nothing changes."""
    S = 4096
    c = _case(S, seed=4)
    dirty = c["GD"].copy()
    dirty[np.arange(N)[None, :] < (np.arange(N)[:, None] // 64) * 64] = np.nan
    t = dict(form=5, N=N, GD=c["GD"], Ta=c["Ta"], Tb=c["Tb"])
    a = ctx.local_score_test(S, directed=True, pairs=c["pairs"], tally=t)
    b = ctx.local_score_test(S, directed=True, pairs=c["pairs"], tally=dict(t, GD=dirty))
    assert not np.any(np.isnan(b["part"])) and np.array_equal(a["part"], b["part"]) and np.array_equal(a["out2"], b["out2"])