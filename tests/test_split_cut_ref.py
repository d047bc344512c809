"""CPU tests of the reference the kernel-level tests of the split's cut stage judge by (tests/split_cut_ref.py): it gives the lists
of the project's oracle for all four rules on groups with and without ties; plain fp64 numpy in another summation order takes the
same branches on every decided task and stays inside the value and mean bounds; five seeded mistakes fall outside; and the data
leave no task undecided in the classes `integer` and `separated` and at most a tenth of any (rule, width, class) cell elsewhere."""
import ctypes as C

import numpy as np
import pytest

import split_cut_ref as sc

RULE_NAMES = tuple(sc.RULES)
FP64_WIDTHS = (1, 5, 65, 129, 257)  # the fp64-in-another-order check; the cap is asserted at every width


def _one_column_group(kind, k, d, rng):
    """(X (k, d) with only column 0 non-zero, w): integers, dyadic weights with exact roots, sum w x = 0 exactly -- the oracle's
    mean is 0 and its principal axis +-e0, so its projections are +-x0 sqrt(w) to the bit"""
    x = rng.integers(-40, 41, k).astype(np.float64)
    w = 4.0 ** rng.integers(-1, 3, k)
    if kind == "ties":  # repeated projections: at the middle, at both ends, in between
        x[rng.integers(0, k, k // 2)] = x[0]
        x[1], w[1] = 2.0 * x[2], w[2] / 4.0  # x sqrt(w) equal, the rows differ
        x[rng.permutation(k)[:2]] = np.abs(x).max() + 1.0
        x[rng.permutation(k)[:2]] = -np.abs(x).max() - 1.0
    w[k - 1] = 1.0
    x[k - 1] = -(w[:k - 1] * x[:k - 1]).sum()
    X = np.zeros((k, d))
    X[:, 0] = x
    return X, w


@pytest.mark.parametrize("rule", RULE_NAMES)
@pytest.mark.parametrize("kind", ["distinct", "ties"])
def test_reference_gives_the_oracle_lists(kind, rule):
    from oracle import oracle as orc

    rng = np.random.default_rng([7, RULE_NAMES.index(rule), kind == "ties"])
    signs = set()
    for k in (3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 100, 257):
        for d in (2, 3):
            X, w = _one_column_group(kind, k, d, rng)
            rows = np.arange(k)
            try:
                low, high = orc.split(X, w, rows + 1, rule)
                got = ("lists", (low - 1).tolist(), (high - 1).tolist())
            except orc.OracleError as e:
                got = ("error", e.rc)
            z0 = X[:, 0] * np.sqrt(w)
            assert np.array_equal(z0 * z0, X[:, 0] ** 2 * w), "the projections are not exact"
            match = []
            for sign in (1.0, -1.0):
                r = sc.split_group(X, w, rows, sign * z0, sc.RULES[rule])
                if r["rc"] == sc.OK:
                    assert r["margin"] > 1.0 or r["margin"] == 0.0  # (exact data: an exact tie of the sums, or far apart)
                mine = ("error", r["rc"]) if r["rc"] == sc.E_HOMOGENEOUS else ("lists", r["low"], r["high"])
                if mine == got:
                    match.append(sign)
            assert match, (rule, kind, k, d, got)
            signs.update(match)
    assert signs  # (either axis direction is a valid eigenvector; one of them is the oracle's)


def test_rss_equal_sums_as_the_oracle():
    """Two groups where a median round meets EQUAL sums (exact data): high absorbs, as in the oracle; the seeded mistake `low
    absorbs on equality` gives other lists"""
    from oracle import oracle as orc

    for x in ([-1.0, 1.0, 4.0, -4.0, 3.0, -3.0], [-5.0, -1.0, 0.0, 2.0, 4.0]):
        k = len(x)
        X = np.zeros((k, 3))
        X[:, 0] = x
        w, rows = np.ones(k), np.arange(k)
        low, high = orc.split(X, w, rows + 1, "rss")
        good = [sc.split_group(X, w, rows, s * X[:, 0], sc.RSS) for s in (1.0, -1.0)]
        bad = [sc.split_group(X, w, rows, s * X[:, 0], sc.RSS, equal_goes_low=True) for s in (1.0, -1.0)]
        lists = ((low - 1).tolist(), (high - 1).tolist())
        assert any((r["low"], r["high"]) == lists for r in good)
        assert not any((r["low"], r["high"]) == lists for r in bad)


@pytest.fixture(scope="module")
def cells():
    return sc.Cells()


@pytest.mark.parametrize("d", sc.WIDTHS)
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_undecided_cap_and_fp64_in_another_order(cells, cls, d):
    for rule in RULE_NAMES:
        X, w, ids, off, z, refs = cells(rule, d, cls)
        share = sc.undecided_share(refs)
        print(f"split_cut_ref {rule} d={d} {cls}: undecided {share:.3f}, tie tasks {sum(r['tie'] for r in refs)}")
        assert share <= (0.0 if cls in ("integer", "separated") else 0.1), (rule, d, cls, share)
        if d not in FP64_WIDTHS:
            continue
        # plain fp64, sums in another order: the same branches on every decided task, values and means inside the bounds
        refs64 = sc.reference_batch(X, w, ids, off, z, sc.RULES[rule], dtype=np.float64)
        verdict = sc.judge(X, w, ids, off, sc.as_output(X, w, ids, off, refs64), refs, direct=rule in ("size", "diameter"))
        print(f"    fp64 numpy: value {verdict['value']:.3f} mean {verdict['mean']:.3f} of the bound")
        assert sc.passes(verdict), (rule, d, cls, verdict)


def test_problem_shapes_are_the_ones_the_kernels_branch_on():
    assert sorted(sc.LENS) == [3, 4, 5, 15, 16, 17, 63, 64, 65, 66, 67, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1031,
                               1032, 1033, 2049, 4096, 4097]
    assert list(sc.LENS) != sorted(sc.LENS)
    assert sorted(sc.group_lengths(5))[-2:] == [32768, 32769] and max(sc.group_lengths(63)) == 4097
    assert max(sc.group_lengths(256)) == 300 and len(sc.group_lengths(256)) == len(sc.LENS)
    seen = set()
    for d in sc.WIDTHS:
        for cls in sc.CLASSES:
            lens = sc.group_lengths(d)
            seen.update((k, sc.z_class_of(t, d, cls)) for t, k in enumerate(lens))
    assert all((k, zc) in seen for k in sc.LENS for zc in sc.Z_CLASSES)
    rng = np.random.default_rng(5)
    for k in (3, 4, 5, 64, 65, 257, 1025):  # the z classes are what their names say
        for rule in (sc.SIZE, sc.DIAMETER):
            z = sc.make_z("ties_at_cut", k, rule, rng)
            assert sc.cut_rule(z, rule == sc.SIZE)[2], (k, rule)
            z = sc.make_z("signed_zero", k, rule, rng)
            low, high, tie = sc.cut_rule(z, rule == sc.SIZE)
            assert tie and (z == 0).any() and (k < 6 or np.signbit(z[z == 0]).any()), (k, rule)
        z = sc.make_z("tie_at_max", k, sc.RSS, rng)
        assert (z == z.max()).sum() >= 2 and (z == z.min()).sum() == 1
        z = sc.make_z("tie_at_min", k, sc.RSS, rng)
        assert (z == z.min()).sum() >= 2 and (z == z.max()).sum() == 1
    found = False
    for seed in range(40):  # even k, two different middle values, a row on their half-sum
        z = sc.make_z("ties_at_cut", 1024, sc.SIZE, np.random.default_rng(seed))
        zs = np.sort(z)
        found |= zs[511] != zs[512] and bool((z == zs[511] / 2.0 + zs[512] / 2.0).any())
    assert found


@pytest.mark.parametrize("mistake", ["tie_le", "upper_median", "sorted_children", "parent_weight"])
def test_a_seeded_mistake_falls_outside(cells, mistake):
    """What a wrong kernel would return: the tie rule with <= ; the even-k median taken as the upper middle value; the children
    lists sorted by id; a mean divided by the parent's weight (rss absorbing on equal sums: test_rss_equal_sums_as_the_oracle)"""
    d, cls = 5, "gaussian"
    rule = {"tie_le": "diameter", "upper_median": "size", "sorted_children": "rss", "parent_weight": "rss2"}[mistake]
    X, w, ids, off, z, refs = cells(rule, d, cls)
    assert sc.passes(sc.judge(X, w, ids, off, sc.as_output(X, w, ids, off, refs), refs))
    if mistake in ("tie_le", "upper_median"):
        wrong = sc.reference_batch(X, w, ids, off, z, sc.RULES[rule], **{mistake: True})
        verdict = sc.judge(X, w, ids, off, sc.as_output(X, w, ids, off, wrong), refs)
        assert verdict["lists_differ"] or verdict["rc_differs"], verdict
    elif mistake == "sorted_children":
        verdict = sc.judge(X, w, ids, off, sc.as_output(X, w, ids, off, refs, sort_children=True), refs)
        assert len(verdict["lists_differ"]) > len(refs) // 2, verdict
    else:
        verdict = sc.judge(X, w, ids, off, sc.as_output(X, w, ids, off, refs, parent_weight=True), refs)
        assert verdict["mean"] > 1.0 and not verdict["lists_differ"], verdict


def test_a_nan_projection_sends_every_row_high():
    z = np.array([3.0, np.nan, 1.0, 2.0, 5.0])
    for median in (True, False):
        low, high, tie = sc.cut_rule(z, median)
        assert low == [] and high == [0, 1, 2, 3, 4] and not tie
    assert sc.split_group(None, None, None, z, sc.SIZE)["rc"] == sc.E_EMPTY_CLUSTER


def test_group_cut_hook_refuses_a_null_context():
    from cge.jl_amd import api

    lib = api.load_library()
    assert lib.cge_group_cut_test(None, None, None, C.c_int64(1), C.c_int(0), None, C.c_int(0), None, None, None, None, None,
                                  None, None, None) == -7
