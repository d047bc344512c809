"""Kernel-level tests of the statistics stage of a landmark split (run with -m gpu on an MI355X): k_group_mean / k_gather_means,
k_group_cov, k_group_eig, k_group_project and k_group_side_sums through the hook cge_group_stats_test -- the split's own batch
builder, chunk tables and launch wrappers -- against long-double references with a-priori error bounds (tests/group_stats_ref.py,
whose own CPU tests show that plain fp64 numpy stays inside them and that a dropped row, ignored weights or a first-chunk mean
fall outside).

One batch per width and data class, groups of 1, 2, 3, 15, 16, 17, 1, 33, 1023, 1024, 1025, 2049 rows in this task order:
several tasks inside one 16-row wave of the projection, a chunk boundary +- 1, three chunks in one task (beyond d = 129 the long
groups stop at 300 rows).  The widths cross every form: the mean's and the side sums' columns per lane (64 / 128 / 256 / 512),
the thread-tile covariance (d < 48), the MFMA SYRK with one diagonal tile (48 .. 128; odd d: the unpaired loads), with
off-diagonal tiles and the tiled merge (d > 128), the chunk's own write of a one-chunk group against the chunk-ordered merge,
both forms of the projection and both device eigen-solvers."""
import numpy as np
import pytest

import group_stats_ref as gs

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 5, 47, 48, 63, 64, 65, 127, 128, 129, 200, 256, 257, 512]
ALONE = (0, 5, 10, 11)  # tasks run again as a batch of their own: 1 row, 17 rows, 1025 rows (two chunks), the longest


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _same_bits(a, b, keys):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in keys)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("cls", gs.CLASSES)
def test_group_stats_against_long_double(ctx, cls, d):
    X, w, ids, off = gs.make_problem(cls, d)
    side = gs.make_sides(d, off)
    ctx.set_vertex_data(np.ones(gs.N_ROWS, dtype=np.int64), w)
    ctx.set_embedding(X)
    T = len(off) - 1

    out = ctx.group_stats_test(ids, off, side=side)
    worst = gs.worst_ratios(X, w, ids, off, out, side)
    print(f"group_stats d={d} {cls} computed_mean " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert gs.is_symmetric(out["cov"]), "cov is not bitwise symmetric"
    assert all(v <= 1.0 for v in worst.values()), worst

    again = ctx.group_stats_test(ids, off, side=side)  # a second call: the same bits
    assert _same_bits(out, again, ("mean", "sw", "cov", "vec", "z", "sums"))

    for t in ALONE:  # a group alone in its batch: the same bits as inside the batch
        one = ctx.group_stats_test(ids[off[t]:off[t + 1]], np.array([0, off[t + 1] - off[t]], dtype=np.int32))
        assert np.array_equal(one["mean"][0], out["mean"][t]) and np.array_equal(one["cov"][0], out["cov"][t]), t
        assert np.array_equal(one["vec"][0], out["vec"][t]) and np.array_equal(one["z"], out["z"][off[t]:off[t + 1]]), t
        assert one["sw"][0] == out["sw"][t]

    # the means are known (a child inherits its mean from the parent's side sums): gathered, not computed
    mean_in = gs.ref_mean(X, w, ids, off)[0].astype(np.float64)
    given = ctx.group_stats_test(ids, off, mean_in=mean_in)
    assert np.array_equal(given["mean"].view(np.int64), mean_in.view(np.int64)) and np.all(np.isnan(given["sw"]))
    worst = gs.worst_ratios(X, w, ids, off, given, None, mean_given=True)
    print(f"group_stats d={d} {cls} given_mean " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert gs.is_symmetric(given["cov"]), "cov is not bitwise symmetric"
    assert all(v <= 1.0 for v in worst.values()), worst
    assert given["cov"].shape == (T, d, d)


def test_group_stats_beyond_512_columns(ctx):
    """d = 513: sixteen columns per lane in the mean, five MFMA tiles a side in the covariance, the host eigen-solver behind the
    device covariance and the projection's general form (the side sums stop at d = 512 and are refused)."""
    from cge.jl_amd import api

    d = 513
    X, w, ids, off = gs.make_problem("integer", d)
    ctx.set_vertex_data(np.ones(gs.N_ROWS, dtype=np.int64), w)
    ctx.set_embedding(X)
    out = ctx.group_stats_test(ids, off)
    worst = gs.worst_ratios(X, w, ids, off, out)
    print(f"group_stats d={d} integer computed_mean " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert gs.is_symmetric(out["cov"]) and all(v <= 1.0 for v in worst.values()), worst
    assert _same_bits(out, ctx.group_stats_test(ids, off), ("mean", "sw", "cov", "vec", "z"))
    with pytest.raises(api.CGEError, match="d <= 512"):
        ctx.group_stats_test(ids, off, side=gs.make_sides(d, off))


def test_group_stats_hook_refuses_bad_groups(ctx):
    from cge.jl_amd import api

    X, w, ids, off = gs.make_problem("integer", 5)
    ctx.set_vertex_data(np.ones(gs.N_ROWS, dtype=np.int64), w)
    ctx.set_embedding(X)
    with pytest.raises(api.CGEError, match="empty group"):
        ctx.group_stats_test(ids[:3], np.array([0, 3, 3], dtype=np.int32))
    with pytest.raises(api.CGEError, match="outside"):
        ctx.group_stats_test(np.array([1, gs.N_ROWS], dtype=np.int32), np.array([0, 2], dtype=np.int32))
    with pytest.raises(api.CGEError, match="two groups"):
        ctx.group_stats_test(np.array([4, 7, 4], dtype=np.int32), np.array([0, 2, 3], dtype=np.int32))
    with pytest.raises(api.CGEError, match="side"):
        ctx.group_stats_test(ids[:3], np.array([0, 3], dtype=np.int32), side=np.array([1, 3, 2], dtype=np.uint8))
