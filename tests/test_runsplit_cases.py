"""CPU tests of the inputs of the driver tests (tests/runsplit_cases.py; the GPU side is tests/test_gpu_runsplit_driver.py): no
decision of any case hangs on the last bits of an eigenvector (the oracle's Jacobi routine and LAPACK's give the same ids and the
same error codes, and so does LAPACK's eigenvector with seeded jitter), the `blocks` and `distinct` cases fail where they are
meant to fail, the `tied` cases really hold groups of equal heap value, and the `forced` cases have the shapes their name promises."""
import numpy as np
import pytest

import runsplit_cases as rc
from oracle import oracle as orc

ALL_CASES = rc.tied_cases() + rc.error_cases() + rc.forced_cases()


@pytest.fixture(scope="module")
def failing():
    """(case name, rule) -> (first failing land, code), from the oracle"""
    return {(c.name, rule): rc.first_failing_land(orc, c, rule) for c in rc.error_cases() for rule in rc.RULES}


def _lands(case, rule, failing):
    if case.lands:
        return case.lands
    land = failing[(case.name, rule)][0]
    return (land - 1, land)


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_jacobi_and_lapack_give_the_same_ids_and_errors(case, failing):
    for rule in rc.RULES:
        for land in _lands(case, rule, failing):
            j = rc.oracle_outcome(orc, case, land, rule)
            l = rc.oracle_outcome(orc, case, land, rule, lapack=True)
            assert rc.same_outcome(j, l), (case, rule, land, j, l)


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_jittered_eigenvectors_give_the_same_ids_and_errors(case, failing):
    """Stronger than two clean routines, which can agree on a degenerate group by producing the same bits: every component of
    LAPACK's eigenvector moved by up to 2^-44, twelve seeds.  (The first `blocks` construction, 150 free points of [-16, 16]^2, passed
    the check above and failed this one, and failed against the oracle on the device in exactly the same cases.)"""
    for rule in rc.RULES:
        for land in _lands(case, rule, failing):
            want = rc.oracle_outcome(orc, case, land, rule)
            for seed in range(1, 13):
                got = rc.oracle_outcome(orc, case, land, rule, jitter=seed)
                assert rc.same_outcome(want, got), (case, rule, land, seed)


@pytest.mark.parametrize("case", rc.error_cases(), ids=repr)
def test_first_failing_land(case, failing):
    """rss refuses a block of equal rows once it is on top of the heap, long before the rows run out; the other rules split such a
    block and fail only when a single row is on top: at land = n + 1, with the code of their own first check"""
    n = case.n
    for rule in rc.RULES:
        land, code = failing[(case.name, rule)]
        print(f"{case} {rule}: first failing land {land} of n = {n}, code {code}")
        assert rc.oracle_outcome(orc, case, land - 1, rule)[0] == "ok"
        if case.name.startswith("blocks") and rule == "rss":
            assert land <= n and code == rc.E_HOMOGENEOUS
            assert land > 2 * max(case.forced, 1) + 50  # a long run of good pops in front of it
        else:
            assert land == n + 1 and code == (rc.E_EMPTY if rule == "diameter" else rc.E_ASSERT)
    if case.name.startswith("blocks"):
        assert 350 <= n <= 420
        P = np.unique(case.X, axis=0)
        assert len(P) == 150 and np.abs(P).max() <= rc.BLOCKS_RANGE and (case.w == 2.0).all()
        assert len(set(P[:, 0] - P[:, 1])) == 150 and len(set(P[:, 0] + P[:, 1])) == 150  # no two points on a common diagonal
        counts = np.unique(case.X, axis=0, return_counts=True)[1]
        assert counts.min() == 1 and counts.max() == 4 and (counts >= 3).sum() >= 30  # homogeneous blocks for rss to refuse


def _group_values(case, ids):
    """per cluster q: the sorted (length, bit pattern of -total_rss) of its groups"""
    out = []
    for cl in case.clusters:
        cl = np.asarray(cl)
        mine = ids[cl - 1]
        rows = []
        for g in np.unique(mine):
            members = np.ascontiguousarray(cl[mine == g])
            v = -orc.total_rss(case.X, case.w, members) if len(members) > 1 else 0.0
            rows.append((len(members), np.float64(v).view(np.int64).item()))
        out.append(sorted(rows))
    return out


@pytest.mark.parametrize("case", rc.tied_cases(), ids=repr)
def test_tied_cases_hold_ties(case):
    """At land = 12 k every cluster has been cut into the same k groups: the same lengths and the same heap values to the bit, so
    the heap held (and holds) groups of more than one row with equal values, twelve at a time"""
    assert case.n == 768 and len(case.clusters) == 12
    seen = 0
    for k in (max(case.forced, 2), 8):
        kind, ids = rc.oracle_outcome(orc, case, 12 * k, "size")
        assert kind == "ok" and ids.max() + 1 == 12 * k
        per = _group_values(case, ids)
        assert all(p == per[0] for p in per[1:]), case
        assert len(per[0]) == k
        seen += sum(1 for length, _ in per[0] if length > 1)
    assert seen >= 2
    if case.d == 1:  # ties among the projections too: a value of the pattern is there more than once
        assert len(np.unique(case.X[:64, 0])) < 64
    else:
        assert len(np.unique(case.X[:64], axis=0)) == 64 and np.abs(case.X[:64]).max() <= 8
        assert np.array_equal(case.X[64:128] - case.X[:64], np.tile([64.0, 0.0, 0.0], (64, 1)))


@pytest.mark.parametrize("case", rc.forced_cases(), ids=repr)
def test_forced_cases_have_their_shapes(case):
    f = case.forced
    lengths = sorted(len(c) for c in case.clusters)
    assert lengths == sorted([1, 2, 3, f, f + 1, 40, 300])
    assert sorted(v for c in case.clusters for v in c) == list(range(1, case.n + 1))
    G = rc.forced_groups(lengths, f)
    assert case.lands == (G - 3, G, G + 5)
    for rule in ("rss2", "size"):
        for land, want in zip(case.lands, (G, G, G + 5)):  # at or below G the global phase has nothing to do
            kind, ids = rc.oracle_outcome(orc, case, land, rule)
            assert kind == "ok" and ids.max() + 1 == want, (case, rule, land)
