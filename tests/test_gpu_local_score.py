"""The local half of the score (elements 5-7 of a score vector, src/divergence.jl:178-213, :485-517) kernel by kernel: the device
sampler, the prepared pairs, full_graph_D of the sampled pairs and the tallies (run with -m gpu on an MI355X).

The stages go through the testing hook cge_local_score_test (the sweep's own functions and launch wrappers); the reference is
tests/local_score_ref.py (Python integers, fp64 dist(), np.longdouble tallies), pinned on the CPU by tests/test_local_score_ref.py
together with every input condition named below.  The exchange variants of options shard_rows / shard_ingest stay with
tests/test_gpu_two_ranks.py, the multi-problem launch with tests/test_gpu_batch.py.

D   draws: n = 48 with edges by a predicate of 75 % density, so that the rejection loop runs 27 rounds at S = 4096 (up to 43
    directed) -- the todo / next ping-pong, attempt numbers, the table re-sized five times, about 3000 duplicate keys in round
    0 and probe runs of 4+ slots; pos, neg_i, neg_j and attempt element for element, both routes, two streams, undirected and
    directed; S = 1 and S = 257 (a thread beyond a workgroup; in round 1 a key probes past the end of its 1024-slot table).  The
    give-up path on 87.5 % density (a sample needs attempt 90): CGE_E_ARG after 64 rounds, and the context draws again.
P   prepare: 30 vertices, rows in both orientations and a self-loop, weighted and unit lists, with and without the overwriting
    draw, undirected and directed; all five outputs exactly.
X   distances: d in {1, 63, 64, 65, 130, 511, 512} x S in {1, 4095, 4096, 4101} (both sides of the switch to the tile kernel at
    4096 pairs, d = 511 its last width, a last workgroup of 5 pairs), rows of mixed magnitudes, pairs with i == j and repeated
    pairs; bit for bit, and the same bits for a pair on either side of the switch.
T1  tallies on exact inputs (alpha 1, distances in {0, .., 3/4}, dyadic T, vw, lweight, weights k / 4): the 64 block tallies and
    {num, den} equal the reference exactly -- forms 1 (also relabelled), 2 and 3, undirected and directed, at S in {1, 255, 16385,
    65535, 65536, 65836, 262401} (one sample; one grid stride and a sample; the wide switch; the wide grid's stride); every slot
    has a weight sum of its own and thousands of samples tie (the same pair twice, and equal products of different factors).
T2  tallies on random inputs (alpha 3.25, distances from the distance stage): every slot's num and den within terms x 2^-53 x
    the slot's weight sum of the long-double reference, no sample with a relative gap below 1e-9.
F4  the epilogue of the fused persistent fit at N = 256 landmarks (the sweep's first fused size) in 3 interleaved communities,
    S in {1, 300, 16385}: the prepared operands exactly; the block tallies == form 1's on the iterate the launch left; num within
    the weight of the samples whose reference gap is below 1e-9; the same bits again and under a start skew; no tally from an
    abandoned launch.
R   every refusal of the hook by its message.

Measured on an MI355X (256 CUs; `-s` prints the figures):
  T2: the largest device error of a slot as a fraction of its bound: 0.0072 (num 0.0039, den 0.0072, at S = 16385).
  F4: the weight share of the samples with a gap below 1e-9: 0 at every S (no sample in the band; the fits took >= 2 iterations).
Scratch mutants of the kernels (tried on a copy, not committed) and the tests that noticed them:
  check_neg_kernel without `attempt[k] += 1`        test_draws_are_the_reference_stream_element_for_element (the draw then
                                                    ends in the give-up error), test_the_sampler_gives_up_.. (its second draw)
  `todo` ignored by a round's two kernels           the same two (2129 of 4096 samples differ; the dense graph no longer gives up)
  `pos >= neg` in the two tally kernels             test_landmark_tallies_on_exact_inputs and test_exact_mode_tallies_on_exact_inputs
                                                    at every S, S = 1 included
  auc_fold_kernel reading `s + q` for               the same two at S >= 65536 (63 of 64 slots), and
  `s * AUC_WIDE + q`                                test_landmark_tallies_on_random_inputs[65836]
  prep_samples_kernel without the (min, max) swap   test_prepared_pairs_and_weights (weighted and unit, at sample 0 of S = 1)
  weights of prep_samples_kernel from pos2          test_prepared_pairs_and_weights[weighted]
  `aden[(vb + 1) & 63]` in the fused epilogue       test_the_fused_fits_epilogue_tally at every S (the den column of the tallies)
  pair_dist_tile_kernel: `ld = d`                   nothing, and nothing can: the rows stay disjoint, the + 1 only staggers the
                                                    LDS banks.  Its pair-to-row map `4 * wv + u` for `wv + 4 * u` instead:
                                                    test_pair_distances_bit_for_bit at every d <= 511
"""
import functools

import numpy as np
import pytest

import fit_ref as fr
import local_score_ref as ls

pytestmark = pytest.mark.gpu

LD = ls.LD
E_ARG = -7
SEED, NV = ls.DRAW_SEED, ls.DRAW_N


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _graph(ctx, rows0, n, w=None):
    rows0 = np.asarray(rows0, np.int64)
    ctx.set_graph(rows0 + 1, np.ones(len(rows0)) if w is None else w, n)


def _ring(ctx, n):
    _graph(ctx, np.stack((np.arange(n), (np.arange(n) + 1) % n), axis=1), n)


_worst = {}


def _note(key, value):
    _worst[key] = max(_worst.get(key, 0.0), float(value))
    print(f"  {key}: largest so far {_worst[key]:.3g}")


# ---- D: draws ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_draw(pred, directed, stream, S):
    m = len(ls.edge_rows(pred, directed))
    return (ls.draw_pos(SEED, stream, S, m),) + ls.draw_neg(SEED, stream, S, NV, pred, directed)


@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
def test_draws_are_the_reference_stream_element_for_element(ctx, directed):
    pred = ls.edge_d if directed else ls.edge_u
    _graph(ctx, ls.edge_rows(pred, directed), NV)
    for stream, S in ((0, 4096), (1, 4096), (0, 1), (0, 257)):
        pos, ni, nj, att = _ref_draw(pred, directed, stream, S)
        if S == 4096:
            assert 8 <= att.max() <= 48  # the input condition: the loop runs far past its first rounds
        outs = [ctx.local_score_test(S, directed=directed, draw=(SEED, stream, route)) for route in (1, 2)]
        for o in outs:
            assert np.array_equal(o["pos"], pos), (stream, S)
            bad = np.flatnonzero((o["neg_i"] != ni) | (o["neg_j"] != nj) | (o["attempt"] != att))
            assert bad.size == 0, (stream, S, bad[:8], o["neg_i"][bad[:8]], o["neg_j"][bad[:8]], o["attempt"][bad[:8]], att[bad[:8]])
            assert o["rounds"] == att.max() + 1
    a, b = _ref_draw(pred, directed, 0, 4096), _ref_draw(pred, directed, 1, 4096)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])  # the second stream is another stream


def test_the_sampler_gives_up_after_64_rounds_and_draws_again(ctx):
    """On (i + j) % 8 != 0 a sample of seed 11 needs attempt 90: an error return after 64 small rounds, not a fault."""
    from cge.jl_amd import api

    _graph(ctx, ls.edge_rows(ls.edge_dense, False), NV)
    for route in (1, 2):
        with pytest.raises(api.CGEError) as e:
            ctx.local_score_test(4096, draw=(SEED, 0, route))
        assert e.value.code == E_ARG and "could not find enough non-edges" in str(e.value), str(e.value)
        pos, ni, nj, att = _ref_draw(ls.edge_dense, False, 0, 400)
        assert 32 <= att.max() < 64
        o = ctx.local_score_test(400, draw=(SEED, 0, route))
        assert np.array_equal(o["pos"], pos) and np.array_equal(o["neg_i"], ni) and np.array_equal(o["neg_j"], nj)
        assert np.array_equal(o["attempt"], att) and o["rounds"] == att.max() + 1


# ---- P: prepare ----------------------------------------------------------------------------------------------------------------
def _prepare_graph(weighted):
    rng = np.random.default_rng(21)
    n = 30
    rows = np.array([(i, j) for i in range(n) for j in range(i + 1, n) if (i * 7 + j * 3) % 5 < 2], np.int64)
    rows = np.concatenate((rows, rows[::3, ::-1], [[4, 4]], rows[1::5, ::-1]))  # both orientations, a self-loop among them
    rows = rows[rng.permutation(len(rows))]
    return n, rows, (rng.integers(1, 40, len(rows)) / 8.0 if weighted else None)


@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unit"])
def test_prepared_pairs_and_weights(ctx, weighted):
    """Pairs from pos2 where there is one, weights from pos, (min, max) when undirected; every output exactly."""
    n, rows, w = _prepare_graph(weighted)
    _graph(ctx, rows, n, w)
    m = len(rows)
    assert np.any(rows[:, 0] > rows[:, 1]) and np.any(rows[:, 0] == rows[:, 1])
    rng = np.random.default_rng(22)
    for S in (1, 257, 1000):
        pos, pos2 = rng.integers(0, m, S), rng.integers(0, m, S)
        ni, nj = rng.integers(0, n, S), rng.integers(0, n, S)
        pos[0], pos2[0] = int(np.flatnonzero(rows[:, 0] > rows[:, 1])[0]), int(np.flatnonzero(rows[:, 0] > rows[:, 1])[1])
        ni[0], nj[0] = 9, 2
        for directed in (False, True):
            for p2 in (None, pos2):
                exp = ls.prepare(rows[:, 0], rows[:, 1], w, pos, p2, ni, nj, directed)
                o = ctx.local_score_test(S, directed=directed, draws=(pos, ni, nj), pos2=p2, prepare=True)
                for key, e in zip(("pi", "pj", "ni", "nj", "wts"), exp):
                    assert np.array_equal(o[key], e), (S, directed, p2 is not None, key)
                if p2 is not None and weighted:
                    assert not np.array_equal(o["wts"], w[pos2])


def test_prepare_takes_the_pairs_just_drawn(ctx):
    rows = ls.edge_rows(ls.edge_u, False)
    w = ((np.arange(len(rows)) * 5) % 23 + 1) / 4.0
    _graph(ctx, rows, NV, w)
    pos, ni, nj, _ = _ref_draw(ls.edge_u, False, 0, 257)
    o = ctx.local_score_test(257, draw=(SEED, 0, 1), prepare=True)
    for key, e in zip(("pi", "pj", "ni", "nj", "wts"), ls.prepare(rows[:, 0], rows[:, 1], w, pos, None, ni, nj, False)):
        assert np.array_equal(o[key], e), key


# ---- X: distances --------------------------------------------------------------------------------------------------------------
DIST_S = [1, 4095, 4096, 4101]


@pytest.mark.parametrize("d", [1, 63, 64, 65, 130, 511, 512])
def test_pair_distances_bit_for_bit(ctx, d):
    """pair_dist_kernel (S < 4096, or d > 511) and pair_dist_tile_kernel (rows of d + 1 doubles in LDS) against dist()."""
    rng = np.random.default_rng(100 + d)
    n = 40
    X = rng.standard_normal((n, d)) * np.exp(rng.normal(size=(n, d)) * 3)
    _ring(ctx, n)
    ctx.set_embedding(X)
    S = max(DIST_S)
    pi, pj, ni, nj = (rng.integers(0, n, S).astype(np.int32) for _ in range(4))
    pj[::7] = pi[::7]  # i == j
    ni[::5], nj[::5] = pi[::5], pj[::5]  # repeated pairs
    pi[S - 5:], pj[S - 5:] = [3, 3, 39, 0, 17], [3, 38, 39, 39, 16]  # the last workgroup of the tile kernel: 5 pairs
    hi = 7.25
    ep, en = ls.dist(X, pi, pj, hi), ls.dist(X, ni, nj, hi)
    assert np.all(ep[::7] == 0) and np.count_nonzero(ep) > S // 2
    got = {}
    for s in DIST_S:
        o = ctx.local_score_test(s, pairs=(pi[:s], pj[:s], ni[:s], nj[:s], np.ones(s)), hi=hi, distances=True)
        for key, e in (("dpos", ep), ("dneg", en)):
            bad = np.flatnonzero(o[key].view(np.uint64) != e[:s].view(np.uint64))
            assert bad.size == 0, (d, s, key, bad[:8], o[key][bad[:8]], e[bad[:8]])
        got[s] = o
    # the two kernels on either side of S = 4096 (d <= 511) give a pair the same bits
    assert np.array_equal(got[4095]["dpos"], got[4096]["dpos"][:4095]) and np.array_equal(got[4096]["dneg"], got[4101]["dneg"][:4096])


# ---- T1: exact tallies ---------------------------------------------------------------------------------------------------------
EXACT_S = [1, 255, 16385, 65535, 65536, 65536 + 300, 262144 + 257]


def _expect_exact(o, pos, neg, wts, what):
    num, den, cnt, (tn, td) = ls.tally(pos, neg, wts)
    part = o["part"]
    bad = np.flatnonzero((part[:, 0] != num.astype(np.float64)) | (part[:, 1] != den.astype(np.float64)))
    assert bad.size == 0, (what, bad[:8], part[bad[:8]], num[bad[:8]], den[bad[:8]])
    assert o["out2"][0] == float(tn) and o["out2"][1] == float(td), (what, o["out2"], tn, td)


@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("S", EXACT_S)
def test_landmark_tallies_on_exact_inputs(ctx, S, directed):
    """auc_landmark_kernel on both grids, auc_fold_kernel, auc_final_kernel and permute_rows_kernel: every block tally exactly."""
    c = ls.exact_landmark_case(S, directed=directed)
    n, N = len(c["v2l"]), c["N"]
    _ring(ctx, n)
    pi, pj, ni, nj, wts = c["pairs"]
    pos = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], pi, pj, c["dists"][0], 1.0)
    neg = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], ni, nj, c["dists"][1], 1.0)
    if S >= 16385:
        assert np.count_nonzero(pos == neg) >= 50  # `>` against `>=` cannot hide
    t = dict(form=1, N=N, alpha=1.0, Ta=c["Ta"], Tb=c["Tb"] if directed else None, v2l=c["v2l"], vw=c["vw"], lweight=c["lweight"])
    o = ctx.local_score_test(S, directed=directed, pairs=c["pairs"], dists=c["dists"], tally=t)
    _expect_exact(o, pos, neg, wts, ("form 1", S, directed))
    # the relabelled route: T in sweep order (communities interleaved in landmark order), un-permuted through old2new
    _, o2n = ls.interleaved_old2new(N, 3)
    Ts, Tsb = np.empty(N), np.empty(N)
    Ts[o2n], Tsb[o2n] = c["Ta"], c["Tb"]
    assert not np.array_equal(Ts, c["Ta"])
    t.update(Ta=Ts, Tb=Tsb if directed else None, old2new=o2n)
    o2 = ctx.local_score_test(S, directed=directed, pairs=c["pairs"], dists=c["dists"], tally=t)
    _expect_exact(o2, pos, neg, wts, ("form 1 relabelled", S, directed))


@pytest.mark.parametrize("S", EXACT_S)
def test_exact_mode_tallies_on_exact_inputs(ctx, S):
    """auc_exact_kernel<false> (undirected and directed) and <true> on the packed tiles of N = 130 (3 tiles per side): every
    block tally exactly, forms 2 and 3 the same bits."""
    for directed in (False, True):
        c = ls.exact_matrix_case(S, directed=directed)
        pi, pj, ni, nj, wts = c["pairs"]
        pos, neg = ls.values_exact(c["GD"], c["Ta"], c["Tb"], pi, pj), ls.values_exact(c["GD"], c["Ta"], c["Tb"], ni, nj)
        if S >= 16385:
            assert np.count_nonzero(pos == neg) >= 50
        t = dict(form=2, N=c["N"], GD=c["GD"], Ta=c["Ta"], Tb=c["Tb"] if directed else None)
        o = ctx.local_score_test(S, directed=directed, pairs=c["pairs"], tally=t)
        _expect_exact(o, pos, neg, wts, ("form 2", S, directed))
        if not directed:
            t["form"] = 3
            o3 = ctx.local_score_test(S, pairs=c["pairs"], tally=t)
            _expect_exact(o3, pos, neg, wts, ("form 3", S))
            assert np.array_equal(o3["part"], o["part"]) and np.array_equal(o3["out2"], o["out2"])


# ---- T2: random inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("S", [1000, 16385, 65536 + 300])
def test_landmark_tallies_on_random_inputs(ctx, S, directed):
    """Per slot |num - ref| and |den - ref| <= terms x 2^-53 x the slot's weight sum: the slot adds `terms` non-negative
    summands of at most that sum, one rounding per addition in any order.  No sample is near a tie (gap >= 1e-9; the device's
    pow is within an ulp and the five products and quotients of a side within 3e-16 each), so every indicator is the
    reference's and the sums differ by their roundings alone."""
    c = ls.random_landmark_case(S, directed=directed)
    n = len(c["v2l"])
    _ring(ctx, n)
    ctx.set_embedding(c["emb"])
    pi, pj, ni, nj, wts = c["pairs"]
    t = dict(form=1, N=c["N"], alpha=c["alpha"], Ta=c["Ta"], Tb=c["Tb"] if directed else None, v2l=c["v2l"], vw=c["vw"],
             lweight=c["lweight"])
    o = ctx.local_score_test(S, directed=directed, pairs=c["pairs"], hi=c["hi"], distances=True, tally=t)
    assert np.array_equal(o["dpos"], ls.dist(c["emb"], pi, pj, c["hi"])) and np.array_equal(o["dneg"], ls.dist(c["emb"], ni, nj, c["hi"]))
    pos = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], pi, pj, o["dpos"], c["alpha"])
    neg = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], ni, nj, o["dneg"], c["alpha"])
    assert ls.gaps(pos, neg).min() >= 1e-9  # the input condition
    num, den, cnt, (tn, td) = ls.tally(pos, neg, wts)
    bound = ls.sum_bound(cnt, den.astype(np.float64))
    en, ed = np.abs(o["part"][:, 0].astype(LD) - num).astype(np.float64), np.abs(o["part"][:, 1].astype(LD) - den).astype(np.float64)
    live = cnt > 0
    print(f"  S = {S}: num error / bound {np.max(en[live] / bound[live]):.3g}, den {np.max(ed[live] / bound[live]):.3g}")
    _note("T2 error / bound", max(np.max(en[live] / bound[live]), np.max(ed[live] / bound[live])))
    assert np.all(en <= bound) and np.all(ed <= bound), (S, np.flatnonzero(en > bound)[:8], np.flatnonzero(ed > bound)[:8])
    assert np.all(o["part"][~live] == 0)
    tot = 64 * 2.0 ** -53 * float(td) + float(bound.sum())  # the 64 slots, then their sum in block order
    assert abs(LD(o["out2"][0]) - tn) <= tot and abs(LD(o["out2"][1]) - td) <= tot


# ---- F4: the epilogue of the fused persistent fit ------------------------------------------------------------------------------
FUSED_N = 256  # the first landmark count a sweep runs the fused chain at (layout_tables); its geometry is asked of the device below


@functools.lru_cache(maxsize=None)
def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _fused_case(S):
    rng = np.random.default_rng(300 + S)
    n, N, d = 700, FUSED_N, 8
    c = dict(n=n, N=N)
    c["emb"] = rng.standard_normal((n, d))
    c["hi"] = float(2.0 * np.sqrt(d) * np.abs(c["emb"]).max() * 1.01)
    c["v2l"] = np.concatenate((np.arange(N), rng.integers(0, N, n - N))).astype(np.int32)
    c["vw"] = rng.random(n) + 0.5
    c["lweight"] = rng.random(N) * 5 + 1
    c["old2new"] = ls.interleaved_old2new(N, 3)[1]
    c["problem"] = fr.random_undirected(N, 2.0, 31)
    pi, pj = ls.random_pairs(rng, S, n, False)
    ni, nj = ls.random_pairs(rng, S, n, False)
    c["pairs"] = (pi, pj, ni, nj, ls.sample_weights(S))
    return c


def _fused_tally(c):
    pr = c["problem"]
    return dict(form=4, N=c["N"], alpha=pr["alpha"], D=pr["D"], w=pr["w"], T0=pr["T0"], eps=0.25, delta=0.001, v2l=c["v2l"],
                vw=c["vw"], lweight=c["lweight"], old2new=c["old2new"])


@pytest.mark.parametrize("S", [1, 300, 16385])
def test_the_fused_fits_epilogue_tally(ctx, S):
    """auc_prepare_kernel and the tally loop of fit_flow_body.inc, launched as a sweep launches them with the tally wanted:
    (a) aidx, afac, aden are the gather through v2l and old2new, exactly; (b) the 64 block tallies equal form 1's on the iterate
    the launch left (the kernel's comment promises auc_landmark_kernel's arithmetic); (c) num against the long-double reference
    on that iterate within the weight of the samples whose reference gap is below 1e-9, that weight at most 1 % of den; (d) the
    same bits on a second run and under a start skew of 20 naps; (e) an abandoned launch is reported and writes no tally."""
    Nt = (FUSED_N + 63) // 64
    assert 4 * Nt <= _cus() and Nt * (Nt + 1) // 2 <= 4 * _cus()  # flow_geometry, fused: one tile per wave, one quarter block per workgroup
    c = _fused_case(S)
    n, N, o2n, v2l = c["n"], c["N"], c["old2new"], c["v2l"]
    _ring(ctx, n)
    ctx.set_embedding(c["emb"])
    pi, pj, ni, nj, wts = c["pairs"]
    o = ctx.local_score_test(S, pairs=c["pairs"], hi=c["hi"], distances=True, tally=_fused_tally(c))
    assert o["status"] == 0 and o["iters"] >= 2 and not np.any(np.isnan(o["T"]))
    # (a)
    for q, v in enumerate((pi, pj, ni, nj)):
        assert np.array_equal(o["aidx"][q], o2n[v2l[v]]), q
        assert np.array_equal(o["afac"][2 * q], c["vw"][v]) and np.array_equal(o["afac"][2 * q + 1], c["lweight"][v2l[v]]), q
    den_slots = np.bincount(ls.slot_of(S, wide=False), weights=wts, minlength=64)  # (dyadic weights: exact in any order)
    assert np.array_equal(o["aden"], den_slots) and np.array_equal(o["part"][:, 1], den_slots)
    assert np.array_equal(o["dpos"], ls.dist(c["emb"], pi, pj, c["hi"]))
    # (b) T comes back in sweep order: form 1 un-permutes it through the same old2new
    t1 = dict(form=1, N=N, alpha=c["problem"]["alpha"], Ta=o["T"], v2l=v2l, vw=c["vw"], lweight=c["lweight"], old2new=o2n)
    f1 = ctx.local_score_test(S, pairs=c["pairs"], dists=(o["dpos"], o["dneg"]), tally=t1)
    assert np.array_equal(o["part"], f1["part"]) and np.array_equal(o["out2"], f1["out2"])
    # (c)
    T = o["T"][o2n]  # by landmark
    pos = ls.values_landmark(T, T, v2l, c["vw"], c["lweight"], pi, pj, o["dpos"], c["problem"]["alpha"])
    neg = ls.values_landmark(T, T, v2l, c["vw"], c["lweight"], ni, nj, o["dneg"], c["problem"]["alpha"])
    num, den, cnt, (tn, td) = ls.tally(pos, neg, wts, wide=False)
    band = float(np.sum(wts[ls.gaps(pos, neg) < 1e-9]))
    _note("F4 in-band weight share", band / float(td))
    assert band <= 0.01 * float(td)
    assert abs(LD(o["out2"][0]) - tn) <= band and o["out2"][1] == float(td)
    assert np.all(np.abs(o["part"][:, 0].astype(LD) - num) <= band)
    # (d)
    again = ctx.local_score_test(S, pairs=c["pairs"], hi=c["hi"], distances=True, tally=_fused_tally(c))
    try:
        ctx.set_option("fit_persistent_test_delay", 20)
        skew = ctx.local_score_test(S, pairs=c["pairs"], hi=c["hi"], distances=True, tally=_fused_tally(c))
    finally:
        ctx.set_option("fit_persistent_test_delay", 0)
    for other in (again, skew):
        assert other["iters"] == o["iters"] and np.array_equal(other["T"], o["T"]) and np.array_equal(other["part"], o["part"])
    # (e)
    try:
        ctx.set_option("fit_persistent_test_timeout", 1)
        gone = ctx.local_score_test(S, pairs=c["pairs"], hi=c["hi"], distances=True, tally=_fused_tally(c))
    finally:
        ctx.set_option("fit_persistent_test_timeout", 0)
    assert gone["status"] == 1 and np.all(np.isnan(gone["part"])) and np.all(np.isnan(gone["out2"])) and np.all(np.isnan(gone["T"]))
    assert np.array_equal(gone["aden"], den_slots)  # (prepared before the launch)


# ---- R: refusals ---------------------------------------------------------------------------------------------------------------
def _refused(ctx, text, *args, **kw):
    from cge.jl_amd import api

    with pytest.raises(api.CGEError) as e:
        ctx.local_score_test(*args, **kw)
    assert e.value.code == E_ARG and "local_score_test" in str(e.value) and text in str(e.value), str(e.value)


def test_refusals():
    """Every CGE_E_ARG of the hook, before any launch, by its message (a context of its own: some need nothing resident).  The
    refusal of a sharded context needs two ranks: test_two_ranks_sharded_rows (tests/test_gpu_two_ranks.py) holds it."""
    from cge.jl_amd import api

    ctx = api.Context(0)
    try:
        S = 8
        z, one = np.zeros(S, np.int32), np.ones(S)
        pairs = (z, z + 1, z, z + 2, one)
        c = ls.exact_landmark_case(S)
        lm = dict(form=1, N=c["N"], alpha=1.0, Ta=c["Ta"], v2l=c["v2l"], vw=c["vw"], lweight=c["lweight"])
        _refused(ctx, "S = 0 samples", 0, draw=(1, 0, 1))
        _refused(ctx, "the graph is not resident", S, draw=(1, 0, 1))
        _refused(ctx, "the graph is not resident", S, draws=(z, z, z + 1), prepare=True)
        _refused(ctx, "nothing is resident", S, pairs=pairs, hi=1.0, distances=True)
        _refused(ctx, "nothing is resident", S, pairs=pairs, dists=(one, one), tally=lm)
        n = len(c["v2l"])
        _ring(ctx, n)
        _refused(ctx, "the embedding is not resident", S, pairs=pairs, hi=1.0, distances=True)
        _refused(ctx, "the embedding is not resident", S, pairs=pairs, tally=lm)  # (form 1 without dists runs the distance stage)
        ctx.set_embedding(np.random.default_rng(0).standard_normal((n, 3)))
        _refused(ctx, "prepared or supplied, not both", S, pairs=pairs, prepare=True, draws=(z, z, z + 1))
        _refused(ctx, "pi_in, pj_in, ni_in, nj_in and wts_in together", S, pairs=(z, z, z, z, None), hi=1.0, distances=True)
        _refused(ctx, "pos_in, neg_i_in and neg_j_in together", S, draws=(z, None, z), prepare=True)
        _refused(ctx, "Prepare takes pos_in", S, prepare=True)
        _refused(ctx, "Prepare takes pos_in", S, hi=1.0, distances=True)  # (no pairs: Prepare would have to make them)
        _refused(ctx, "pos2_in goes with Prepare", S, pairs=pairs, pos2=z, hi=1.0, distances=True)
        _refused(ctx, "dpos_in and dneg_in go together", S, pairs=pairs, dists=(one, None), tally=lm)
        _refused(ctx, "go with a tally", S, pairs=pairs, dists=(one, one))
        _refused(ctx, "hi = 0", S, pairs=pairs, hi=0.0, distances=True)
        _refused(ctx, f"pos_in[3] = {n} outside 0..{n - 1}", S, draws=(np.where(np.arange(S) == 3, n, 0), z, z + 1), prepare=True)
        _refused(ctx, "pos_in[0] = -1", S, draws=(z - 1, z, z + 1), prepare=True)
        _refused(ctx, f"neg_j_in[7] = {n}", S, draws=(z, z, np.where(np.arange(S) == 7, n, 1)), prepare=True)
        _refused(ctx, "pos2_in[0] = -1", S, draws=(z, z, z + 1), pos2=z - 1, prepare=True)
        _refused(ctx, f"pj_in[0] = {n}", S, pairs=(z, z + n, z, z + 1, one), hi=1.0, distances=True)
        _refused(ctx, "ni_in[0] = -1", S, pairs=(z, z + 1, z - 1, z + 1, one), dists=(one, one), tally=lm)
        _refused(ctx, "N = 0", S, pairs=pairs, dists=(one, one), tally=dict(lm, N=0))
        _refused(ctx, "N = 46341", S, pairs=pairs, dists=(one, one), tally=dict(lm, N=46341))
        _refused(ctx, "take v2l, vw and lweight", S, pairs=pairs, dists=(one, one), tally=dict(lm, vw=None))
        _refused(ctx, f"v2l[2] = {c['N']}", S, pairs=pairs, dists=(one, one), tally=dict(lm, v2l=np.where(np.arange(n) == 2, c["N"], c["v2l"])))
        o2n = np.arange(c["N"], dtype=np.int32)
        _refused(ctx, "old2new[1] = -1", S, pairs=pairs, dists=(one, one), tally=dict(lm, old2new=np.where(o2n == 1, -1, o2n)))
        _refused(ctx, "not a permutation (5 twice)", S, pairs=pairs, dists=(one, one), tally=dict(lm, old2new=np.where(o2n == 6, 5, o2n)))
        _refused(ctx, "form 1 takes Ta", S, pairs=pairs, dists=(one, one), tally=dict(lm, Ta=None))
        ex = ls.exact_matrix_case(S)
        em = dict(form=2, N=ex["N"], GD=ex["GD"], Ta=ex["Ta"])
        _refused(ctx, "forms 2 and 3 take GD and Ta", S, pairs=pairs, tally=dict(em, GD=None))
        _refused(ctx, f"pi_in[0] = {ex['N']} outside 0..{ex['N'] - 1}", S, pairs=(z + ex["N"], z, z, z + 1, one), tally=em)
        _refused(ctx, f"forms 2 and 3 on prepared pairs take N = n (N = {ex['N']}, n = {n})", S, draws=(z, z, z + 1), tally=em)
        _refused(ctx, "form 3 is undirected only", S, directed=True, pairs=pairs, tally=dict(em, form=3))
        pr = fr.random_undirected(FUSED_N, 2.0, 31)
        f4 = dict(lm, form=4, N=FUSED_N, D=pr["D"], w=pr["w"], T0=pr["T0"], lweight=np.ones(FUSED_N))
        _refused(ctx, "form 4 is undirected only", S, directed=True, pairs=pairs, dists=(one, one), tally=f4)
        _refused(ctx, "form 4 takes D, w and T0", S, pairs=pairs, dists=(one, one), tally=dict(f4, T0=None))
        _refused(ctx, "eps > 0 and delta >= 0", S, pairs=pairs, dists=(one, one), tally=dict(f4, eps=0.0))
        _refused(ctx, "eps > 0 and delta >= 0", S, pairs=pairs, dists=(one, one), tally=dict(f4, delta=-1.0))
        big = 64 * (_cus() // 4) + 1  # 4 Nt > the CU count: a workgroup would reduce two quarter blocks
        prb = dict(D=np.zeros((big, big)), w=np.ones(big), T0=np.ones(big))
        _refused(ctx, f"the geometry of the fused persistent fit declines N = {big}", S, pairs=pairs, dists=(one, one),
                 tally=dict(f4, N=big, lweight=np.ones(big), **prb))
        try:
            ctx.set_option("pow_exp2", 0)
            _refused(ctx, "pow_exp2", S, pairs=pairs, dists=(one, one), tally=f4)
        finally:
            ctx.set_option("pow_exp2", 1)
    finally:
        ctx.close()
