"""The plain reference of the local score's kernel tests (tests/local_score_ref.py), pinned on the CPU: the stream against the
library's host draw, dist() against the oracle's, the tallies against a literal loop over src/divergence.jl:185-213 -- and every
input condition tests/test_gpu_local_score.py relies on (attempt counts, duplicate keys and probe runs, ties, gaps, distinct slot
sums), so that a change to a generator or to a seed fails here first."""
import ctypes as C
import functools

import numpy as np
import pytest

import local_score_ref as ls

LD = ls.LD


# ---- the stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stream, m", [(11, 0, 846), (11, 1, 846), (42, 1003, 1), (-1, 7, 2 ** 31 - 1), (2 ** 62 + 5, 2, 613)])
def test_positive_draws_are_the_librarys(seed, stream, m):
    from cge.jl_amd import api

    S = 500
    got = np.zeros(S, np.int64)
    rc = api.load_library().cge_host_pos_draw(C.c_int64(seed), C.c_int64(stream), C.c_int64(S), C.c_int64(m), got.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert np.array_equal(ls.draw_pos(seed, stream, S, m) + 1, got)


def test_a_sample_depends_on_seed_stream_k_and_attempt_alone():
    ni, nj, att = ls.draw_neg(ls.DRAW_SEED, 0, 300, ls.DRAW_N, ls.edge_u, False)
    ni2, nj2, att2 = ls.draw_neg(ls.DRAW_SEED, 0, 40, ls.DRAW_N, ls.edge_u, False)
    assert np.array_equal(ni[:40], ni2) and np.array_equal(nj[:40], nj2) and np.array_equal(att[:40], att2)
    assert np.all(ni < nj) and not any(ls.edge_u(i, j) for i, j in zip(ni, nj))
    for k in (0, 7, 299):  # the accepted pair is attempt att[k]'s candidate, every earlier one is an edge
        assert ls.candidate(ls.DRAW_SEED, 0, k, int(att[k]), ls.DRAW_N, False) == (ni[k], nj[k])
        assert all(ls.edge_u(*ls.candidate(ls.DRAW_SEED, 0, k, a, ls.DRAW_N, False)) for a in range(int(att[k])))
    di, dj, _ = ls.draw_neg(ls.DRAW_SEED, 0, 300, ls.DRAW_N, ls.edge_d, True)
    assert np.all(di != dj) and np.any(di > dj) and not any(ls.edge_d(i, j) for i, j in zip(di, dj))


@functools.lru_cache(maxsize=None)
def _draw(pred, directed, stream, S):
    return ls.draw_neg(ls.DRAW_SEED, stream, S, ls.DRAW_N, pred, directed)


def test_the_draw_cases_run_the_rejection_loop_deep():
    """Seed 11, stream 0, S = 4096 on (i + j) % 4 != 0: at most 26 attempts beyond the first for any sample, 12 365 rejections."""
    _, _, att = _draw(ls.edge_u, False, 0, 4096)
    assert att.max() == 26 and att.sum() == 12365
    for pred, directed, stream in ((ls.edge_u, False, 0), (ls.edge_u, False, 1), (ls.edge_d, True, 0)):
        _, _, att = _draw(pred, directed, stream, 4096)
        assert 8 <= att.max() <= 48
        tabs = ls.round_tables(ls.DRAW_SEED, stream, ls.DRAW_N, directed, att)
        assert len(tabs) == att.max() + 1 and tabs[0]["cnt"] == 4096 and tabs[0]["size"] == 16384
        assert tabs[0]["distinct"] <= 48 * 47 // (1 if directed else 2)
        assert tabs[0]["duplicates"] >= 1800  # 1128 (2256) distinct pairs under 4096 samples: the `old == key` branch
        assert max(t["longest"] for t in tabs) >= 4 and sum(t["displaced"] for t in tabs) >= 100  # probe runs
        assert len({t["size"] for t in tabs}) >= 4  # the table is re-sized with the shrinking todo list
    # S = 257: one thread beyond a workgroup; in round 1 a key is pushed past the end of the 1024-slot table to its start
    _, _, att = _draw(ls.edge_u, False, 0, 257)
    tabs = ls.round_tables(ls.DRAW_SEED, 0, ls.DRAW_N, False, att)
    assert att.max() >= 8 and tabs[1]["wrapped"] >= 1 and tabs[0]["size"] == 2048 and all(t["size"] == 1024 for t in tabs[1:])
    assert ls.draw_neg(ls.DRAW_SEED, 0, 1, ls.DRAW_N, ls.edge_u, False)[2][0] == 1  # S = 1 takes a second round too


def test_the_dense_graph_holds_a_sample_beyond_64_rounds():
    _, _, att = _draw(ls.edge_dense, False, 0, 4096)
    assert att.max() == 90 and np.count_nonzero(att >= 64) == 3  # attempt number 90: the sampler gives up after attempts 0 .. 63


def test_edge_rows_store_both_orientations():
    rows = ls.edge_rows(ls.edge_u, False)
    assert len(rows) == sum(ls.edge_u(i, j) for i in range(48) for j in range(i + 1, 48))
    assert np.any(rows[:, 0] > rows[:, 1]) and np.any(rows[:, 0] < rows[:, 1])
    d = ls.edge_rows(ls.edge_d, True)
    s = set(map(tuple, d.tolist()))
    assert any((j, i) not in s for i, j in s) and 0.7 < len(d) / (48 * 47) < 0.8


# ---- prepared pairs --------------------------------------------------------------------------------------------------------------
def test_prepare_by_hand():
    src, dst, w = np.array([5, 1, 3, 2]), np.array([2, 4, 3, 0]), np.array([0.5, 1.5, 2.5, 3.5])
    pos, pos2, ni, nj = np.array([0, 2, 3]), np.array([1, 0, 0]), np.array([4, 0, 2]), np.array([1, 3, 2])
    a, b, u, v, wt = ls.prepare(src, dst, w, pos, None, ni, nj, False)
    assert (a.tolist(), b.tolist(), u.tolist(), v.tolist(), wt.tolist()) == ([2, 3, 0], [5, 3, 2], [1, 0, 2], [4, 3, 2], [0.5, 2.5, 3.5])
    a, b, u, v, wt = ls.prepare(src, dst, w, pos, pos2, ni, nj, True)  # pairs of pos2, weights of pos, no swap
    assert (a.tolist(), b.tolist(), u.tolist(), v.tolist(), wt.tolist()) == ([1, 5, 5], [4, 2, 2], [4, 0, 2], [1, 3, 2], [0.5, 2.5, 3.5])
    assert ls.prepare(src, dst, None, pos, None, ni, nj, True)[4].tolist() == [1.0, 1.0, 1.0]


# ---- dist() ----------------------------------------------------------------------------------------------------------------------
def test_dist_is_the_oracles_bit_for_bit(test115):
    from oracle import oracle as orc

    emb = np.asarray(test115["embedding"], dtype=np.float64)
    n, d = emb.shape
    L = orc.lib()
    L.orc_dist.restype = C.c_double
    L.orc_dist.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]
    _, flat = orc._f(emb)
    rng = np.random.default_rng(0)
    i, j = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    i[:50] = j[:50]
    exp = np.array([L.orc_dist(int(a) + 1, int(b) + 1, orc._ptr(flat), n, d) for a, b in zip(i, j)])
    got = ls.dist(emb, i, j, 1.0)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)) and np.all(got[:50] == 0.0) and np.all(got[50:][i[50:] != j[50:]] > 0)
    assert np.array_equal(ls.dist(emb, i, j, 3.7), exp / 3.7)
    # mixed magnitudes, where the order of the additions shows: the ascending sum, not numpy's pairwise one
    X = emb * np.exp(rng.normal(size=emb.shape) * 6)
    _, flat = orc._f(X)
    exp = np.array([L.orc_dist(int(a) + 1, int(b) + 1, orc._ptr(flat), n, d) for a, b in zip(i, j)])
    assert np.array_equal(ls.dist(X, i, j, 1.0), exp)


# ---- the tallies -----------------------------------------------------------------------------------------------------------------
def test_tallies_against_the_literal_loop_on_30_vertices():
    """src/divergence.jl:185-213 word for word (1-based, the packed triangle of idx()), in fp64, on continuous inputs."""
    rng = np.random.default_rng(4)
    n, N, S, alpha = 30, 6, 200, 2.75
    v_to_l = np.concatenate((np.arange(N), rng.integers(0, N, n - N))) + 1
    init_vw, vweights, T = rng.random(n) + 0.5, rng.random(N) + 1, rng.random(N) + 0.5

    def idx(nn, i, j):
        return nn * (i - 1) - (i - 1) * (i - 2) // 2 + (j - i + 1)

    fgD = rng.random(n * (n + 1) // 2 + 1)
    E = [(int(min(a, b)), int(max(a, b)), float(w)) for a, b, w in zip(rng.integers(1, n + 1, S), rng.integers(1, n + 1, S), rng.random(S) + 0.1)]
    NE = [(int(min(a, b)), int(max(a, b))) for a, b in zip(rng.integers(1, n + 1, S), rng.integers(1, n + 1, S))]
    pos, neg, aw = np.zeros(S), np.zeros(S), np.zeros(S)
    for ind, (i, j, w) in enumerate(E):
        adj_Ti = T[v_to_l[i - 1] - 1] * init_vw[i - 1] / vweights[v_to_l[i - 1] - 1]
        adj_Tj = T[v_to_l[j - 1] - 1] * init_vw[j - 1] / vweights[v_to_l[j - 1] - 1]
        pos[ind] = adj_Ti * adj_Tj * ((1 - fgD[idx(n, i, j)]) ** alpha)
        aw[ind] = w
    for ind, (i, j) in enumerate(NE):
        adj_Ti = T[v_to_l[i - 1] - 1] * init_vw[i - 1] / vweights[v_to_l[i - 1] - 1]
        adj_Tj = T[v_to_l[j - 1] - 1] * init_vw[j - 1] / vweights[v_to_l[j - 1] - 1]
        neg[ind] = adj_Ti * adj_Tj * ((1 - fgD[idx(n, i, j)]) ** alpha)
    auc = 1 - np.sum((pos > neg) * aw) / np.sum(aw)
    pi, pj = np.array([e[0] for e in E]) - 1, np.array([e[1] for e in E]) - 1
    ni, nj = np.array([e[0] for e in NE]) - 1, np.array([e[1] for e in NE]) - 1
    dpos, dneg = np.array([fgD[idx(n, i, j)] for i, j, _ in E]), np.array([fgD[idx(n, i, j)] for i, j in NE])
    rp = ls.values_landmark(T, T, v_to_l - 1, init_vw, vweights, pi, pj, dpos, alpha)
    rn = ls.values_landmark(T, T, v_to_l - 1, init_vw, vweights, ni, nj, dneg, alpha)
    assert np.allclose(np.float64(rp), pos, rtol=1e-14, atol=0) and np.allclose(np.float64(rn), neg, rtol=1e-14, atol=0)
    assert ls.gaps(rp, rn).min() > 1e-9 and np.array_equal(rp > rn, pos > neg)
    num, den, cnt, (tn, td) = ls.tally(rp, rn, aw)
    assert cnt[0] == S and cnt[1:].sum() == 0 and float(1 - tn / td) == pytest.approx(auc, rel=1e-14)
    # exact mode: P[idx] = T_i T_j GD[idx] (:174), pos and neg read P (:203-210)
    Tn = rng.random(n) + 0.5
    GD = np.zeros((n, n))
    for i in range(1, n + 1):
        for j in range(i, n + 1):
            GD[i - 1, j - 1] = GD[j - 1, i - 1] = fgD[idx(n, i, j)]
    P = {idx(n, i, j): Tn[i - 1] * Tn[j - 1] * fgD[idx(n, i, j)] for i in range(1, n + 1) for j in range(i, n + 1)}
    pos = np.array([P[idx(n, i, j)] for i, j, _ in E])
    neg = np.array([P[idx(n, i, j)] for i, j in NE])
    rp, rn = ls.values_exact(GD, Tn, Tn, pi, pj), ls.values_exact(GD, Tn, Tn, ni, nj)
    assert np.allclose(np.float64(rp), pos, rtol=1e-15, atol=0) and np.array_equal(rp > rn, pos > neg)
    _, _, _, (tn, td) = ls.tally(rp, rn, aw)
    assert float(tn / td) == pytest.approx(np.sum((pos > neg) * aw) / np.sum(aw), rel=1e-14)


def test_slots_of_the_two_grids():
    s = ls.slot_of(16385)
    assert s[0] == s[255] == 0 and s[256] == 1 and s[16383] == 63 and s[16384] == 0  # one grid stride and one sample
    assert np.array_equal(ls.slot_of(65535), ls.slot_of(65536, wide=False)[:65535]) and ls.slot_of(65535)[-1] == 63
    w = ls.slot_of(65536 + 300)
    assert w[0] == w[4095] == 0 and w[4096] == 1 and w[65535] == 15 and w[65536] == 16 and w[-1] == 16
    w = ls.slot_of(262144 + 257)  # the wide grid's stride: 1024 blocks of 256
    assert w[262143] == 63 and w[262144] == 0 and w[-1] == 0


EXACT_S = [1, 255, 16385, 65535, 65536, 65536 + 300, 262144 + 257]


@pytest.mark.parametrize("S", EXACT_S)
def test_the_exact_tier_is_exact_and_full_of_ties(S):
    for directed in (False, True):
        c = ls.exact_landmark_case(S, directed=directed)
        pi, pj, ni, nj, wts = c["pairs"]
        dpos, dneg = c["dists"]
        pos = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], pi, pj, dpos, 1.0)
        neg = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], ni, nj, dneg, 1.0)
        m = ls.exact_matrix_case(S, directed=directed)
        mp = ls.values_exact(m["GD"], m["Ta"], m["Tb"], *m["pairs"][:2])
        mn = ls.values_exact(m["GD"], m["Ta"], m["Tb"], *m["pairs"][2:4])
        for p, q, pairs, planted_same in ((pos, neg, c["pairs"], True), (mp, mn, m["pairs"], False)):
            assert np.array_equal(p.astype(np.float64).astype(LD), p) and np.array_equal(q.astype(np.float64).astype(LD), q)  # fp64 holds them
            assert p[0] == q[0]  # sample 0 is a planted tie: at S = 1 the tally is {0, w_0}
            ties = p == q
            same = (pairs[0] == pairs[2]) & (pairs[1] == pairs[3])
            if S >= 16385:
                assert np.count_nonzero(ties & same) >= 50 and np.count_nonzero(ties & ~same & (p > 0)) >= 50
                assert np.count_nonzero(p > q) >= S // 8 and np.count_nonzero(p < q) >= S // 8
            num, den, cnt, (tn, td) = ls.tally(p, q, pairs[4])
            assert np.array_equal(num.astype(np.float64).astype(LD), num) and float(td) * 4 == int(float(td) * 4) < 2 ** 50
            live = cnt > 0
            assert len(set(den[live].astype(np.float64).tolist())) == live.sum()  # no two slots with the same weight sum
        if not directed:
            assert np.all(c["pairs"][0] < c["pairs"][1]) and np.all(m["pairs"][0] < m["pairs"][1])


RANDOM_S = [1000, 16385, 65536 + 300]


@pytest.mark.parametrize("S", RANDOM_S)
def test_the_random_tier_has_no_near_ties(S):
    for directed in (False, True):
        c = ls.random_landmark_case(S, directed=directed)
        pi, pj, ni, nj, wts = c["pairs"]
        dpos, dneg = ls.dist(c["emb"], pi, pj, c["hi"]), ls.dist(c["emb"], ni, nj, c["hi"])
        assert 0 < dpos.min() and dpos.max() < 1 and dneg.max() < 1
        pos = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], pi, pj, dpos, c["alpha"])
        neg = ls.values_landmark(c["Ta"], c["Tb"], c["v2l"], c["vw"], c["lweight"], ni, nj, dneg, c["alpha"])
        assert ls.gaps(pos, neg).min() >= 1e-9
        num, den, cnt, _ = ls.tally(pos, neg, wts)
        assert np.all(num[cnt > 0] > 0) and np.all(num[cnt > 0] < den[cnt > 0])


def test_interleaved_relabelling():
    comm, o2n = ls.interleaved_old2new(256, 3)
    assert sorted(o2n.tolist()) == list(range(256)) and np.any(o2n != np.arange(256))
    new_comm = np.empty(256, np.int64)
    new_comm[o2n] = comm
    assert np.all(np.diff(new_comm) >= 0) and o2n[0] == 0 and o2n[3] == 1 and o2n[1] == 86
