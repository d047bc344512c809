"""The long-double Chung-Lu reference of tests/test_gpu_fit.py, pinned on the CPU: known answers of the iteration itself, and
every precondition the GPU tests rely on, so that a change to a generator or to a case table fails here first."""
import numpy as np
import pytest

import fit_ref as fr

LD = fr.LD


def test_two_by_two_step_by_hand():
    GD = np.array([[1.0, 0.5], [0.5, 1.0]])
    # undirected: S = T_i sum_j T_j g_ij = (1 (1 + 1), 2 (0.5 + 2)) = (2, 5); w = (3, 4), eps = 1/4
    for dtype in (LD, np.float64):
        r = fr.fit_undirected(GD, [1.0, 2.0], [3.0, 4.0], 0.25, steps=1, dtype=dtype)
        assert np.array_equal(r["S"][0], [2.0, 5.0]) and r["f"][0] == 1.0
        assert np.allclose(np.float64(r["T"][1]), [1.0 + 0.25 * (1.5 - 1.0), 2.0 + 0.5 * (0.8 - 1.0)], rtol=1e-15, atol=0)
        # directed, the diagonal term twice: Sin = (1 (2 * 3 + 0.5 * 1), 2 (0.5 * 3 + 2 * 1)) = (6.5, 7),
        # Sout = (3 (2 * 1 + 0.5 * 2), 1 (0.5 * 1 + 2 * 2)) = (9, 4.5); deg_in = (13, 7), deg_out = (9, 9), eps = 1/2
        d = fr.fit_directed(GD, [1.0, 2.0], [3.0, 1.0], [13.0, 7.0], [9.0, 9.0], 0.5, steps=2, dtype=dtype)
        assert np.array_equal(d["S"][0][0], [6.5, 7.0]) and np.array_equal(d["S"][0][1], [9.0, 4.5])
        assert np.array_equal(d["T"][1][0], [1.5, 2.0]) and np.array_equal(d["T"][1][1], [3.0, 1.5])
        assert d["f"][0] == 6.5 and d["eps"][0] == 0.5
        assert d["eps"][1] == dtype(0.5) * dtype(0.99)  # f_0 = 6.5 > diff = 1.0: the second step moves with the decayed epsilon


@pytest.mark.parametrize("N", [1, 2, 65, 300])
def test_a_constructed_fixed_point_ends_at_the_first_iteration(N):
    pr = fr.random_undirected(N, 2.0, 7)
    GD = (1.0 - pr["D"]) ** 2.0
    rng = np.random.default_rng(8)
    Ts = np.exp(rng.normal(size=N))
    w = (LD(Ts) * (GD.astype(LD) @ LD(Ts))).astype(np.float64)
    for dtype in (LD, np.float64):
        r = fr.fit_undirected(GD, Ts, w, 0.25, delta=1e-9, dtype=dtype)
        assert r["iters"] == 1 and r["f"][0] <= 4 * N * 2.0 ** -53 * np.max(w)
        assert fr.rel_dist(r["T"][1], Ts) <= 0.25 * 4 * N * 2.0 ** -53
    Ti, To = np.exp(rng.normal(size=N)), np.exp(rng.normal(size=N))
    d = np.diagonal(GD).astype(LD)
    din = (LD(Ti) * (GD.astype(LD) @ LD(To) + d * LD(To))).astype(np.float64)
    dout = (LD(To) * (GD.astype(LD) @ LD(Ti) + d * LD(Ti))).astype(np.float64)
    for dtype in (LD, np.float64):
        r = fr.fit_directed(GD, Ti, To, din, dout, 0.9, delta=1e-9, dtype=dtype)
        assert r["iters"] == 1 and fr.rel_dist(np.concatenate(r["T"][1]), np.concatenate((Ti, To))) <= 0.9 * 4 * N * 2.0 ** -53


def test_the_fp64_iteration_adds_in_the_oracle_order():
    """The pair loop of oracle/cge_oracle.c:851-856 and :1034-1041, literally, against the vectorised fp64 sums."""
    rng = np.random.default_rng(5)
    N = 131
    GD = fr.symmetric(rng.random((N, N)))
    T, Ti, To = rng.random(N) + 0.5, rng.random(N) + 0.5, rng.random(N) + 0.5
    S, Sin, Sout = np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        for j in range(i, N):
            tmp = T[i] * T[j] * GD[i, j]
            S[i] += tmp
            if i != j:
                S[j] += tmp
            t1, t2 = Ti[i] * To[j] * GD[i, j], Ti[j] * To[i] * GD[i, j]
            Sin[i] += t1; Sin[j] += t2
            Sout[i] += t2; Sout[j] += t1
    assert np.array_equal(fr.sums_undirected(GD, T, np.float64), S)
    a, b = fr.sums_directed(GD, Ti, To, np.float64)
    assert np.array_equal(a, Sin) and np.array_equal(b, Sout)
    assert fr.rel_dist(fr.sums_undirected(GD.astype(LD), LD(T), LD), S) < N * 2.0 ** -53
    a, b = fr.sums_directed(GD.astype(LD), LD(Ti), LD(To), LD)
    assert fr.rel_dist(a, Sin) < N * 2.0 ** -53 and fr.rel_dist(b, Sout) < N * 2.0 ** -53


def test_zero_degree_rows_keep_their_start_and_stay_out_of_f():
    N = 40
    pr = fr.random_directed(N, 1.0, 3)
    din, dout = pr["w"].copy(), pr["w2"].copy()
    din[[1, 7]] = 0.0
    dout[[2, 7]] = 0.0  # row 7: both zero; 1 and 2: one each
    Tin0, Tout0 = np.full(N, 1.25), np.full(N, 0.75)
    Tin0[1], Tout0[2], Tin0[7], Tout0[7] = 3.0, 5.0, 70.0, 110.0
    GD = 1.0 - pr["D"]
    for dtype in (LD, np.float64):
        r = fr.fit_directed(GD, Tin0, Tout0, din, dout, 0.9, steps=6, dtype=dtype)
        for Tin, Tout in r["T"]:
            assert Tin[1] == 3.0 and Tin[7] == 70.0 and Tout[2] == 5.0 and Tout[7] == 110.0
        Sin, Sout = r["S"][0]
        # |0 - S| of row 7 would be the maximum, and yet f_0 is the maximum over the rows with a positive degree only
        mi, mo = din > 0, dout > 0
        assert Sin[7] > 2 * r["f"][0] and Sout[7] > 2 * r["f"][0]
        assert r["f"][0] == max(np.max(np.abs(dtype(1) * din[mi] - Sin[mi])), np.max(np.abs(dtype(1) * dout[mo] - Sout[mo])))
        assert all(np.any(r["T"][k + 1][0] != r["T"][k][0]) for k in range(6))


def test_zero_weight_rows_of_the_undirected_fit_shrink_by_one_minus_eps():
    pr = fr.random_undirected(65, 1.0, 101)
    z = np.flatnonzero(pr["w"] == 0)
    assert z.size == 2
    r = fr.fit_undirected(1.0 - pr["D"], pr["T0"], pr["w"], 0.25, steps=10)
    assert np.array_equal(np.float64(r["T"][10][z]), [0.75 ** 10] * 2)


def test_exact_problems_are_exact():
    """V1's inputs: one step in fp64 and in long double give the same numbers, whatever the order of the additions."""
    for N in (1, 2, 7, 65, 130):
        for directed in (False, True):
            pr, T1, f0 = fr.exact_problem(N, 40 + N, directed)
            GD = 1.0 - pr["D"]
            assert set(np.unique(pr["D"])) <= {0.0, 0.25, 0.5, 0.75, 1.0} and np.array_equal(pr["D"], pr["D"].T)
            if directed:
                for dtype in (LD, np.float64):
                    r = fr.fit_directed(GD, pr["T0"], pr["T0b"], pr["w"], pr["w2"], 0.5, steps=1, dtype=dtype)
                    assert np.array_equal(r["T"][1][0], T1[0]) and np.array_equal(r["T"][1][1], T1[1]) and r["f"][0] == f0
                if N >= 8:
                    assert np.array_equal(T1[0][[1, 3]], pr["T0"][[1, 3]]) and np.array_equal(T1[1][[2, 5]], pr["T0b"][[2, 5]])
                    assert np.all(pr["w"][[1, 3]] == 0) and np.all(pr["w2"][[2, 5]] == 0)
            else:
                for dtype in (LD, np.float64):
                    r = fr.fit_undirected(GD[::-1, ::-1], pr["T0"][::-1], pr["w"][::-1], 0.25, steps=1, dtype=dtype)  # (another order)
                    assert np.array_equal(r["T"][1], T1[::-1]) and r["f"][0] == f0
            if N > 1:
                assert f0 > 0


@pytest.mark.parametrize("N", [65, 130, 700, 1985])
def test_preconditions_of_the_k_step_cases(N):
    """What test_gpu_fit.py's V3 asserts again on the device's own power matrix: the two values of f that bracket every delta
    are a factor 1.1 apart, the designated directed case decays epsilon at least three times before K and not at every
    iteration, the K of the undirected chains walk every residue of the rings."""
    und, drc = fr.chain_cases(N, False, fr.numpy_gd), fr.chain_cases(N, True, fr.numpy_gd)
    for c in und + drc:
        assert c["gap"] >= fr.GAP and c["A"] >= 2.0 and c["ref"]["iters"] == c["K"]
        f = [float(x) for x in c["ref"]["f"]]
        assert all(x > c["delta"] for x in f[:-1]) and f[-1] <= c["delta"]
    if N <= 700:
        f = [float(x) for x in und[0]["ref"]["f"]]  # from ones: monotone, by 1.3 per iteration at least, 1e-3 near iteration 45
        assert all(a >= 1.3 * b for a, b in zip(f, f[1:])) and 38 <= und[0]["K"] <= 50
    if N == 65:
        Ks = {c["K"] for c in und}
        assert {k % 12 for k in Ks} == set(range(12)) and {1, 2, 3 + 1, 13} <= Ks
        assert und[1]["K"] == 1 and und[1]["start"] == "prev" and not np.all(und[1]["problem"]["T0"] == 1.0)
    if N == fr.DESIGNATED_DIRECTED:
        c = drc[0]
        assert len(c["decays"]) >= 3 and len(c["decays"]) < c["K"] - 1
        f = [float(x) for x in c["ref"]["f"]]
        assert f[1] > f[0] and f[2] < f[0]  # the zig-zag: the decay branch and the running minimum are both live
    assert sum(c["start"] == "prev" for c in und) * 2 >= len(und)
    assert sum(c["start"] == "prev" for c in drc) * 2 >= len(drc)


@pytest.mark.parametrize("N", sorted(fr.SMALL_CHIP_UNDIRECTED_CHAINS))
def test_preconditions_of_the_small_chip_cases(N):
    """The chains of tests/test_gpu_small_chip_fits.py (the sizes of 2 .. 64 CUs): the same preconditions, and what that file asks of
    a chain -- a start that is not the sweep's, a case of three iterations or more (every slot of the rings of 2 and 3 written)."""
    tables = (fr.SMALL_CHIP_UNDIRECTED_CHAINS, fr.SMALL_CHIP_DIRECTED_CHAINS)
    assert sorted(tables[0]) == sorted(tables[1]) and not set(tables[0]) & set(fr.UNDIRECTED_CHAINS)
    for directed in (False, True):
        cases = fr.chain_cases(N, directed, fr.numpy_gd, tables)
        for c in cases:
            assert c["gap"] >= fr.GAP and c["A"] >= 2.0 and c["ref"]["iters"] == c["K"]
            f = [float(x) for x in c["ref"]["f"]]
            assert all(x > c["delta"] for x in f[:-1]) and f[-1] <= c["delta"]
        assert any(c["start"] == "prev" for c in cases) and any(c["K"] >= 3 for c in cases)
        if directed:
            assert any(c["decays"] for c in cases)  # the decaying step size is live


def test_the_chain_tables_cover_the_ring_residues_and_the_issue_s_counts():
    Ks = set()
    for N in (65, 130, 700):
        Ks |= {c["K"] for c in fr.chain_cases(N, False, fr.numpy_gd)}
    assert {2, 3, 4, 5, 13, 25} <= Ks and any(k >= 38 for k in Ks)
    for mod in (2, 3, 4, 12):
        assert {k % mod for k in Ks} == set(range(mod))


def test_step_bound_scale():
    """The a-priori bound of one step is about 2e-14 relative at N = 130 and 1e-12 at N = 4032; a dropped term of a row (1 / N
    of it) is orders of magnitude outside."""
    for N, lo, hi in ((130, 5e-15, 4e-14), (4032, 1e-13, 1.2e-12)):
        T = np.ones(N)
        b = fr.step_bound(0.25, T, 2.0 * T, T, 1.25 * T, N)
        assert lo < float(b[0]) / 1.25 < hi and float(b[0]) < 1e-3 * 0.25 / N
