"""CPU tests of the references the kernel-level landmark tests judge by (tests/group_stats_ref.py, tests/eig_matrices.py): plain
fp64 numpy stays inside every a-priori bound on every data class, three seeded mistakes fall outside them, and the product's
host eigen-solver passes every matrix family under the criterion the device solvers are held to."""
import ctypes as C

import numpy as np
import pytest

import eig_matrices as em
import group_stats_ref as gs


@pytest.mark.parametrize("d", [5, 64, 129])
@pytest.mark.parametrize("cls", gs.CLASSES)
def test_numpy_fp64_is_inside_every_bound(cls, d):
    X, w, ids, off = gs.make_problem(cls, d)
    side = gs.make_sides(d, off)
    out = gs.numpy_stats(X, w, ids, off, side)
    worst = gs.worst_ratios(X, w, ids, off, out, side)
    print(cls, d, {k: round(v, 3) for k, v in worst.items()})
    assert gs.is_symmetric(out["cov"]) and all(v <= 1.0 for v in worst.values()), worst
    mean_in = gs.ref_mean(X, w, ids, off)[0].astype(np.float64)
    out = gs.numpy_stats(X, w, ids, off, None, mean_in)
    worst = gs.worst_ratios(X, w, ids, off, out, None, mean_given=True)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_problem_shapes_are_the_ones_the_kernels_branch_on():
    X, w, ids, off = gs.make_problem("wide_weights", 129)
    assert list(np.diff(off)) == list(gs.LENS) and len(np.unique(ids)) == len(ids) == 5209 and ids.max() < gs.N_ROWS
    assert (w == 0).sum() > 100 and all(w[ids[off[t]:off[t + 1]]].sum() > 0 for t in range(len(gs.LENS)))
    assert max(gs.group_lengths(200)) == 300 and gs.group_lengths(200)[:8] == list(gs.LENS[:8])
    side = gs.make_sides(129, off)
    assert set(side[off[3]:off[4]]) == {1} and set(side[off[4]:off[5]]) == {2} and side[0] == 0
    X, _, ids, off = gs.make_problem("identical_rows", 5)
    assert all((X[ids[off[t]:off[t + 1]]] == X[ids[off[t]]]).all() for t in range(len(gs.LENS)))
    X = gs.make_problem("zero_columns", 5)[0]
    assert ((X == 0).all(0)).sum() == 3


@pytest.mark.parametrize("mutation", ["drop_last_row", "unit_weights", "first_chunk_mean"])
def test_a_seeded_mistake_falls_outside_the_bounds(mutation):
    """What a wrong kernel would return: the 1025-row group (task 10) without its last row; every weight taken as 1; the
    covariance centred with the mean of the group's first chunk (1024 rows) only."""
    d = 64
    X, w, ids, off = gs.make_problem("integer", d)
    side = gs.make_sides(d, off)
    good = gs.numpy_stats(X, w, ids, off, side)
    assert all(v <= 1.0 for v in gs.worst_ratios(X, w, ids, off, good, side).values())
    t = 10
    r = ids[off[t]:off[t + 1]]
    bad = {k: (None if v is None else v.copy()) for k, v in good.items()}
    if mutation == "drop_last_row":
        sub = gs.numpy_stats(X, w, r[:-1].copy(), np.array([0, len(r) - 1], dtype=np.int32), side[off[t]:off[t + 1] - 1])
        for key in ("mean", "sw", "cov", "vec", "sums"):
            bad[key][t] = sub[key][0]
        expect = ("sw", "mean", "cov", "ss", "s", "ws")  # (every z is still the projection on the RETURNED mean and vector)
    elif mutation == "unit_weights":
        bad = gs.numpy_stats(X, np.ones_like(w), ids, off, side)
        expect = ("sw", "mean", "cov", "z", "ss", "s", "ws")
    else:
        y = (X[r] - (X[r[:1024]] * w[r[:1024], None]).sum(0) / w[r[:1024]].sum()) * np.sqrt(w[r])[:, None]
        c = y.T @ y
        bad["cov"][t] = np.triu(c) + np.triu(c, 1).T
        expect = ("cov",)
    worst = gs.worst_ratios(X, w, ids, off, bad, side)
    for key in expect:
        assert worst[key] > 1.0, (mutation, key, worst)


def test_group_stats_hook_refuses_a_null_context():
    from cge.jl_amd import api

    lib = api.load_library()
    assert lib.cge_group_stats_test(None, None, None, C.c_int64(1), None, None, None, None, None, None, None, None) == -7


HOST_WIDTHS = [2, 3, 4, 8, 17, 32, 33, 64, 65, 100, 128, 129, 200, 256]


@pytest.mark.parametrize("d", HOST_WIDTHS)
def test_host_solver_passes_every_family(d):
    from cge.jl_amd import api

    lib = api.load_library()
    worst = 0.0
    for name in em.FAMILIES:
        a = em.family_matrix(name, d)
        v = np.zeros(d)
        assert lib.cge_host_eig_top(a.ctypes.data_as(C.c_void_p), C.c_int64(d), v.ctypes.data_as(C.c_void_p)) == 0
        res, dfc, _, _, fails = em.judge(a, v)
        worst = max(worst, res, dfc)
        assert not fails, (name, d, fails)
    print(f"host solver, d = {d}: worst residual / deficit {worst:.2f} U")
