"""The statistics stage of a landmark split keeps its BITS (run with -m gpu on an MI355X): cov, vec, z and mean of the hook
cge_group_stats_test against SHA-256 digests recorded from the library before the covariance SYRK was cut into half-tile work
units launched longest first and the multisection loop was taken off the LDS (tests/golden/split_stats_bits.npz, recorded by
tests/make_split_stats_bits_fixture.py, which also defines the problems; its `provenance` names the commit).  Neither change
touches an arithmetic operation, an operand order or a summation order, so nothing but equality is accepted.

  * every data class of group_stats_ref at d = 48, 63, 64, 65, 127, 128: groups of 1 .. 2049 rows across the 16-row padding, a
    chunk boundary +- 1 and three chunks in a task; partial tiles and the unpaired loads of odd d;
  * a scheduling case at d = 64 and 128: about 2000 groups of 1 .. 60 rows and five of 1024 .. 3000 rows in one batch -- more
    work units than are resident at once, of very unequal length.  Per task equal to the fixture, equal with the tasks in
    reversed order, and each long group alone equal to itself inside the batch: which workgroup ran when cannot matter;
  * eigen-solver edge cases at d = 2, 3, 64, 65, 128: exactly diagonal small-integer covariances (the Sturm recurrence meets
    q == 0.0 and substitutes the pivot; test_edge_diagonals_meet_a_zero_pivot shows on the CPU that they do) and a zero matrix
    (the degenerate exit)."""
import os

import numpy as np
import pytest

import group_stats_ref as gs
import make_split_stats_bits_fixture as mk

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_stats_bits.npz")


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture
def own_ctx():
    """a context of its own: a context keeps the number of rows of its first table, and these tables have other sizes"""
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return mk.load_fixture(FIXTURE)


def _check(fx, prefix, out):
    bad = [k for k in mk.KEYS if not np.array_equal(mk.digest(out[k]), fx[f"{prefix}/{k}"])]
    assert not bad, f"{prefix}: {bad} differ from the recorded bits ({fx['provenance']})"


@pytest.mark.gpu
@pytest.mark.parametrize("d", mk.CLASS_WIDTHS)
@pytest.mark.parametrize("cls", gs.CLASSES)
def test_class_problems_keep_their_bits(ctx, fx, cls, d):
    X, w, ids, off = gs.make_problem(cls, d)
    mk.load(ctx, X, w)
    _check(fx, f"class/{cls}/{d}", ctx.group_stats_test(ids, off))


@pytest.mark.gpu
@pytest.mark.parametrize("d", mk.SCHED_WIDTHS)
def test_scheduling_case_keeps_its_bits_in_any_order(own_ctx, fx, d):
    ctx = own_ctx
    X, w, ids, off = mk.sched_problem(d)
    mk.load(ctx, X, w)
    T = len(off) - 1
    out = ctx.group_stats_test(ids, off)
    tags = mk.task_tags(out, off)
    differ = np.flatnonzero(tags != fx[f"sched/{d}/task_tags"])
    assert differ.size == 0, f"tasks {differ[:10].tolist()} (of {differ.size}) differ from the recorded bits"
    _check(fx, f"sched/{d}", out)

    # the same groups, last task first: every chunk gets another number, another place in the launch order, another workgroup
    lens = np.diff(off)
    roff = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.int32)
    rids = np.concatenate([ids[off[t]:off[t + 1]] for t in range(T - 1, -1, -1)])
    rev = ctx.group_stats_test(rids, roff)
    for k in ("cov", "vec", "mean"):
        assert np.array_equal(rev[k][::-1].view(np.int64), out[k].view(np.int64)), k
    rz = np.concatenate([rev["z"][roff[T - 1 - t]:roff[T - t]] for t in range(T)])
    assert np.array_equal(rz.view(np.int64), out["z"].view(np.int64))

    long_tasks = mk.sched_long_tasks(off)
    assert len(long_tasks) == len(mk.SCHED_LONG)
    for t in long_tasks:  # a long group alone in its batch: the bits it has inside the batch
        one = ctx.group_stats_test(ids[off[t]:off[t + 1]], np.array([0, lens[t]], dtype=np.int32))
        assert np.array_equal(one["cov"][0].view(np.int64), out["cov"][t].view(np.int64)), t
        assert np.array_equal(one["vec"][0].view(np.int64), out["vec"][t].view(np.int64)), t
        assert np.array_equal(one["mean"][0].view(np.int64), out["mean"][t].view(np.int64)), t
        assert np.array_equal(one["z"].view(np.int64), out["z"][off[t]:off[t + 1]].view(np.int64)), t


@pytest.mark.gpu
@pytest.mark.parametrize("d", mk.EDGE_WIDTHS)
def test_eigen_edge_cases_keep_their_bits(own_ctx, fx, d):
    ctx = own_ctx
    X, w, ids, off = mk.edge_problem(d)
    mk.load(ctx, X, w)
    out = ctx.group_stats_test(ids, off)
    for t, (k, wt) in enumerate(mk.edge_diagonals(d)):  # the construction holds: an exactly diagonal integer matrix, mean 0
        assert np.array_equal(out["cov"][t], np.diag(2.0 * wt * k * k)), t
        assert not out["mean"][t].any(), t
    assert not out["cov"][-1].any(), "identical rows: the zero matrix"
    _check(fx, f"edge/{d}", out)


@pytest.mark.parametrize("d", mk.EDGE_WIDTHS)
def test_edge_diagonals_meet_a_zero_pivot(d):
    """CPU: the multisection on the edge cases' diagonals does meet q == 0.0 (the case they were built for)"""
    assert any(mk.sturm_meets_zero(2.0 * wt * k * k) for k, wt in mk.edge_diagonals(d))
