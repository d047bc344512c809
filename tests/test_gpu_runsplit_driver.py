"""Tests of runsplit's host driver (run with -m gpu on an MI355X): the layer of landmarks_host.cpp between the split's stages, which
have kernel-level tests of their own, and the whole landmarks() runs, which see it on random data of ordinary shape only --
advance_heaps with its speculative tree expansion (the `<=` of its two thresholds, the `take` cut and its 512 rule), the replay in
the reference's pop order, the errors of speculative splits that are held back until (and unless) the group is popped, the forced
phase, the merge with its singletons of short clusters, and the final index.

The inputs are tests/runsplit_cases.py (pinned on the CPU by tests/test_runsplit_cases.py): integer coordinates and power-of-two
weights, so that every heap value is exact and groups tie exactly.  Every comparison is equality of integers or of error codes,
against the oracle's runsplit where the oracle is affordable and device against device -- the testing knob test_lm_speculate
(include/cge_hip_testing.h), whose value 1 is the reference's own order, one split per round -- at the widths where it is not."""
import time

import numpy as np
import pytest

import runsplit_cases as rc

pytestmark = pytest.mark.gpu

KNOBS = (0, 1, 2, 3)
STATS = ("landmark_batches", "landmark_batch_rows", "landmark_splits", "landmark_pops", "landmark_splits_failed", "landmark_take_rounded")
MESSAGES = {rc.E_ASSERT: "AssertionError: size(m, 1) > 1", rc.E_HOMOGENEOUS: "Trying to split homogenous cluster",
            rc.E_EMPTY: "Unexpected empty cluster generated"}  # what throw_rc says


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


def _load(ctx, case):
    ctx.set_inputs(case.edges, np.ones(1), case.w, case.comm, case.X)
    return ctx


def _run(ctx, case, land, rule, knob=0, forced=None):
    """(outcome, stats) of one runsplit under a value of the knob"""
    ctx.set_option("test_lm_speculate", knob)
    try:
        out = rc.outcome(ctx.runsplit, case.clusters, land, case.forced if forced is None else forced, rule)
    finally:
        ctx.set_option("test_lm_speculate", 0)
    return out, {k: ctx.get_stat(k) for k in STATS}


def _check_stats(knob, out, st, where):
    assert st["landmark_splits"] >= st["landmark_pops"], (where, st)  # a group is popped only behind its split
    if knob == 1 and out[0] == "ok":
        assert st["landmark_splits"] == st["landmark_pops"], (where, st)  # nothing wasted: every split was of a top
    if knob in (1, 2):
        assert st["landmark_take_rounded"] == 0, (where, st)
    if out[0] == "ok":
        assert st["landmark_splits_failed"] == 0 or knob != 1, (where, st)  # a failed split of a top is raised


def _all_knobs_against(ctx, case, land, rule, want, where):
    """knob 0 gives `want`; the other values give what 0 gives.  Returns the stats per knob"""
    stats = {}
    base = None
    for knob in KNOBS:
        out, st = _run(ctx, case, land, rule, knob)
        if knob == 0:
            assert rc.same_outcome(out, want), (where, out, want)
            base = out
        assert rc.same_outcome(out, base), (where, knob, out, base)
        _check_stats(knob, out, st, (where, knob))
        stats[knob] = st
        if out[0] == "ok":  # the replay is the same sequence of pops whatever was split ahead of it
            assert st["landmark_pops"] == stats[0]["landmark_pops"], (where, knob, st)
    return base, stats


@pytest.mark.parametrize("rule", rc.RULES)
@pytest.mark.parametrize("case", rc.tied_cases(), ids=repr)
def test_ties_between_groups(ctx, orc, case, rule):
    """Twelve clusters that repeat each other's heap values at every level of the tree (and, at d = 1, rows that repeat each
    other's projections): the reference's sift rules and the `<=` of both thresholds of advance_heaps decide the ids exactly here"""
    _load(ctx, case)
    for land in case.lands:
        want = rc.oracle_outcome(orc, case, land, rule)
        out, stats = _all_knobs_against(ctx, case, land, rule, want, (case, rule, land))
        if out[0] == "ok" and land >= 100:  # (below, the global phase has at most one pop to do: a round either way)
            assert stats[0]["landmark_batches"] < stats[1]["landmark_batches"], (case, rule, land, stats)
        assert stats[0]["landmark_batches"] <= stats[1]["landmark_batches"]


@pytest.mark.parametrize("rule", rc.RULES)
@pytest.mark.parametrize("case", rc.error_cases(), ids=repr)
def test_error_timing(ctx, orc, case, rule):
    """The run fails exactly where the reference fails, with the reference's code: one landmark below, the ids are the oracle's --
    although under rss the speculation has by then split homogeneous blocks and holds their errors back -- and at the first
    failing `land` the call raises.  The context is as good as new afterwards.  What every value of the knob must agree on is
    checked first, the oracle's ids last."""
    from cge.jl_amd import api

    _load(ctx, case)
    land, code = rc.first_failing_land(orc, case, rule)
    good = rc.oracle_outcome(orc, case, land - 1, rule)
    assert good[0] == "ok"
    base = None
    for knob in KNOBS:
        where = (case, rule, land, knob)
        out, st = _run(ctx, case, land - 1, rule, knob)
        base = out if knob == 0 else base
        assert out[0] == "ok" and rc.same_outcome(out, base), where
        _check_stats(knob, out, st, where)
        print(f"runsplit driver {case} {rule} land {land - 1} knob {knob}: " + " ".join(f"{k[9:]} {v}" for k, v in st.items()))
        if rule == "rss" and knob in (0, 2):
            if case.name.startswith("blocks"):  # the deferred error, really exercised
                assert st["landmark_splits_failed"] > 0, where
            else:  # distinct rows: only a single row fails, and a single row is split only on top of the heap
                assert st["landmark_splits_failed"] == 0, where
        ctx.set_option("test_lm_speculate", knob)
        try:
            with pytest.raises(api.CGEError) as e:
                ctx.runsplit(case.clusters, land, case.forced, rule)
        finally:
            ctx.set_option("test_lm_speculate", 0)
        assert e.value.code == code and MESSAGES[code] in str(e.value), (where, str(e.value))
        assert isinstance(e.value, AssertionError) == (code == rc.E_ASSERT)
        again, st2 = _run(ctx, case, land - 1, rule, knob)
        assert rc.same_outcome(again, base) and st2 == st, (where, st, st2)
    assert rc.same_outcome(base, good), (case, rule, land)


@pytest.mark.parametrize("rule", rc.RULES)
@pytest.mark.parametrize("case", rc.forced_cases(), ids=repr)
def test_forced_phase_and_small_clusters(ctx, orc, case, rule):
    """Clusters of 1, 2, 3, forced and forced + 1 rows beside two long ones, handed over unsorted: the local heaps, the singletons
    merge_into_global makes of the short clusters, and `land` at, below and above the number of groups the forced phase leaves"""
    _load(ctx, case)
    for land in case.lands:
        want = rc.oracle_outcome(orc, case, land, rule)
        _all_knobs_against(ctx, case, land, rule, want, (case, rule, land))


WIDE_N, WIDE_LAND = 4000, 2000


def _wide(d):
    rng = np.random.default_rng([11, d])
    X = rng.standard_normal((WIDE_N, d))
    clusters = [list(range(q * 500 + 1, (q + 1) * 500 + 1)) for q in range(8)]
    return rc.Case(f"wide-d{d}", X, np.ones(WIDE_N), clusters, 1, (WIDE_LAND,))


@pytest.mark.parametrize("rule", ["rss", "size"])
@pytest.mark.parametrize("d", [64, 65, 128, 129, 130])
def test_wide_branches_device_against_device(ctx, d, rule):
    """The speculation shares (40 % up to d = 128, 25 % beyond, 10 % for size / diameter) and the 512 rule of 64 < d <= 128, with
    their fence-posts: 1992 pops are outstanding when the global phase starts.  No oracle (minutes at these widths): the ids of the
    default run against those of knob 1, the reference's order, and of knob 2"""
    case = _wide(d)
    _load(ctx, case)
    res = {}
    for knob in (0, 1, 2):
        t0 = time.perf_counter()
        out, st = _run(ctx, case, WIDE_LAND, rule, knob)
        dt = time.perf_counter() - t0
        print(f"runsplit driver wide d={d} {rule} knob {knob}: {dt:.3f} s " + " ".join(f"{k[9:]} {v}" for k, v in st.items()))
        assert out[0] == "ok" and out[1].max() + 1 == WIDE_LAND, (d, rule, knob, out)
        _check_stats(knob, out, st, (d, rule, knob))
        assert st["landmark_pops"] == WIDE_LAND - 8  # forced = 1 leaves the eight clusters as they are: a pop per further landmark
        res[knob] = (out, st)
    for knob in (1, 2):
        assert np.array_equal(res[knob][0][1], res[0][0][1]), (d, rule, knob)
    assert res[0][1]["landmark_batches"] < res[1][1]["landmark_batches"]
    rounded = res[0][1]["landmark_take_rounded"]
    if rule == "rss" and d in (65, 128):  # 40 % of 1992 = 796 > 512: cut down to 512 in the first round at least
        assert rounded > 0, (d, rounded)
    else:
        # d = 64, 129, 130: outside 64 < d <= 128.  size: the share is 10 %, at most 199 of the 1992 outstanding pops, so `take` is
        # the floor of min(remaining, 256) <= 256 and never passes 512: the rule has nothing to round at this `land`
        assert rounded == 0, (d, rule, rounded)


def test_reuse_of_a_context(ctx):
    """Two calls in a row: the same ids and the same stats.  A tied run behind a wide one, in arenas the wide run has grown and
    filled: the ids and stats of the same run on a fresh context"""
    from cge.jl_amd import api

    wide, tied = _wide(65), rc.tied(3, 2)
    _load(ctx, wide)
    a = _run(ctx, wide, WIDE_LAND, "rss")
    b = _run(ctx, wide, WIDE_LAND, "rss")
    assert rc.same_outcome(a[0], b[0]) and a[0][0] == "ok" and a[1] == b[1]
    _load(ctx, tied)
    after = [_run(ctx, tied, land, rule) for rule in rc.RULES for land in (400, tied.n)]
    fresh = api.Context(0)
    try:
        _load(fresh, tied)
        alone = [_run(fresh, tied, land, rule) for rule in rc.RULES for land in (400, tied.n)]
    finally:
        fresh.close()
    for x, y in zip(after, alone):
        assert rc.same_outcome(x[0], y[0]) and x[1] == y[1]


def test_knob_refusals(ctx):
    from cge.jl_amd import api

    for bad in (-1, 4):
        with pytest.raises(api.CGEError) as e:
            ctx.set_option("test_lm_speculate", bad)
        assert e.value.code == -7
