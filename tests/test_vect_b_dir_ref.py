"""tests/vect_b_dir_ref.py on the CPU: its shapes are what the GPU test says they are, its reference is the definition's double
loop, and its check notices a wrong bin."""
import numpy as np
import pytest

import vect_b_dir_ref as vr


@pytest.mark.parametrize("shape", sorted(vr.SHAPES))
def test_shapes(shape):
    N, C = shape
    sizes = vr.SHAPES[shape]
    assert sum(sizes) == N and len(sizes) == C and N >= 256 and C >= 2
    edges = np.cumsum([0] + sizes)
    # a community straddles a 64-vertex boundary of the community-sorted order
    assert any(a // 64 != (b - 1) // 64 for a, b in zip(edges[:-1], edges[1:]) if b > a)
    # at most 64 ids in a 64-vertex block: the tiles accept the layout
    sorted_comm = np.repeat(np.arange(C), sizes)
    assert max(sorted_comm[min(N, b + 64) - 1] - sorted_comm[b] + 1 for b in range(0, N, 64)) <= 64
    if shape in ((321, 12), (700, 30)):
        assert 0 in sizes  # an id without a member


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_reference_is_the_double_loop(kind):
    pr = vr.problem(257, 5, kind, 7)
    N, C = pr["N"], pr["C"]
    assert np.array_equal(pr["GD"], pr["GD"].T) and pr["ref"].shape == (C * C,)
    Z = np.zeros((C, C), vr.LD)
    Ta, Tb, GD, c0 = vr.LD(pr["Ta"]), vr.LD(pr["Tb"]), vr.LD(pr["GD"]), pr["comm"] - 1
    for i in range(N):
        row = (Ta[i] * Tb) * GD[i]
        for q in range(C):
            Z[c0[i], q] += row[c0 == q].sum()
    if kind == "exact":
        assert np.array_equal(pr["ref"], Z.ravel().astype(np.float64))
        assert np.any(pr["Ta"] == 0) and np.any(pr["Tb"] == 0)
    else:
        assert np.allclose(np.asarray(pr["ref"], np.float64), np.asarray(Z.ravel(), np.float64), rtol=1e-15)
        assert pr["nk"].sum() == N * N
    vr.check(pr, np.asarray(pr["ref"], np.float64), "itself")


def test_check_notices_a_wrong_bin_and_an_empty_one_that_is_not_zero():
    pr = vr.problem(321, 12, "random", 3)
    good = np.asarray(pr["ref"], np.float64)
    assert np.count_nonzero(pr["nk"] == 0) == 2 * 12 - 1  # the row and the column of the id without a member
    for k, v in ((5, good[5] * (1 + 1e-12)), (int(np.flatnonzero(pr["nk"] == 0)[0]), 1e-300), (7, np.nan)):
        bad = good.copy()
        bad[k] = v
        with pytest.raises(AssertionError):
            vr.check(pr, bad, "mutant")
    ex = vr.problem(256, 2, "exact", 3)
    bad = ex["ref"].copy()
    bad[1] += 1.0 / 16
    with pytest.raises(AssertionError):
        vr.check(ex, bad, "mutant")
