"""Kernel-level tests of the cut stage of a landmark split (run with -m gpu on an MI355X): the per-group sort, the rule's
one-dimensional cut and the children's lists, values and means -- scan_write / scan_chunk_offsets / rss_rounds<1|2|4|8> /
rss_child_keys / sort_children and the generic host path behind them (rss), rss2_chain_lds + rss2_merge against rss2_walk<1..8>
(rss2), cut_sides + side_values_means (size, diameter) -- through the hook cge_group_cut_test on projections the TEST supplies, so
that ties, chunk boundaries and the orders of equal values sit where the code branches.  Judged by tests/split_cut_ref.py: a
long-double evaluation of the rules with a-priori bounds and per-task margins (its own CPU tests: tests/test_split_cut_ref.py).

One batch per (rule, width, data class); the groups' lengths (task order mixed) are 3 4 5 15 16 17 63..67 127..129 255..257 1023
1024 1025 1031 1032 1033 2049 4096 4097, and 32768, 32769 at d <= 5 (beyond d = 129 they stop at 300 rows).  The per-group sort
picks its form per batch: the batches of d > 5 (longest group 4097 rows) take one or two LDS pieces + the rank merge; the batches of
d <= 5 (longest group 32769) two device-wide rocPRIM sorts; the 32768-row group alone in its batch the piece limit, 8 pieces + the
rank merge; 32769 rows among many short groups rocPRIM's segmented sort (test_long_group_among_many_short_ones).  The z classes
(distinct, ties_at_cut, all_equal, tie_at_max, tie_at_min, two_values, signed_zero) go round the tasks so that every length meets
every class.  Always: the children partition the group, nlow matches, values and means are within their bounds of the long-double
ones of the RETURNED children, a one-row child has DBL_EPSILON, the tie counter is exact, a second call and a task alone in its
batch give the same bits.  Decided tasks (every margin above 1): rc and the lists, order included, are the reference's."""
import numpy as np
import pytest

import split_cut_ref as sc

pytestmark = pytest.mark.gpu

RULE_NAMES = tuple(sc.RULES)
BITS = ("rc", "nlow", "children", "vlow", "vhigh", "cmeans", "route")
# tasks run again as a batch of their own.  32768 (d <= 5) is then the longest group of its batch: the sort's piece limit, 8 LDS
# pieces + the rank merge, against the device-wide rocPRIM sorts the same group gets inside the cell's batch
ALONE_LENS = (3, 66, 1025, 4097, 32768, 32769)


@pytest.fixture(scope="module")
def ctx():
    """one context per number of resident rows (a context keeps its vertex count): ~78 k rows at d <= 5, ~18 k up to d = 129,
    ~6 k beyond -- the resident embedding stays about as long as the groups"""
    from cge.jl_amd import api

    made = {}

    def get(n):
        if n not in made:
            made[n] = api.Context(0)
        return made[n]

    yield get
    for c in made.values():
        c.set_option("test_rss2_one_kernel", 0)
        c.close()


@pytest.fixture(scope="module")
def cells():
    return sc.Cells()


def _load(ctx, X, w):
    c = ctx(len(w))
    c.set_vertex_data(np.ones(len(w), dtype=np.int64), w)
    c.set_embedding(X)
    return c


def _canon(out, off):
    """the outputs as bit patterns; the children range of a failed task holds nothing (whatever the arena held before)"""
    o = {k: np.array(out[k], copy=True) for k in BITS}
    for t in np.flatnonzero(o["rc"] != sc.OK):
        o["children"][off[t]:off[t + 1]] = -1
    o["ties"] = np.array([out["ties"]])
    return {k: (v.view(np.int64) if v.dtype == np.float64 else v) for k, v in o.items()}


def _same(a, b, off, keys=BITS + ("ties",)):
    a, b = _canon(a, off), _canon(b, off)
    return [k for k in keys if not np.array_equal(a[k], b[k])]


def _check_cap(refs, rule, d, cls):
    share = sc.undecided_share(refs)
    assert share <= (0.0 if cls in ("integer", "separated") else 0.1), (rule, d, cls, share)
    return share


def _expected_route(z, off, t):
    """rss: the sorted form declines a task whose maximum is tied (the arg-max is then not the last rank); all-equal is homogeneous"""
    zt = z[off[t]:off[t + 1]]
    return int((zt == zt.max()).sum() > 1 and zt.min() != zt.max())


@pytest.mark.parametrize("d", sc.WIDTHS)
@pytest.mark.parametrize("cls", sc.CLASSES)
def test_cut_stage_against_long_double(ctx, cells, cls, d):
    ctx = _load(ctx, *cells("rss", d, cls)[:2])
    ctx.set_option("test_rss2_one_kernel", 0)
    for rule in RULE_NAMES:
        X, w, ids, off, z, refs = cells(rule, d, cls)
        T, code = len(off) - 1, sc.RULES[rule]
        share = _check_cap(refs, rule, d, cls)
        out = ctx.group_cut_test(ids, off, code, z)
        bounds = np.full((T, 2), np.nan, dtype=sc.LD)
        verdict = sc.judge(X, w, ids, off, out, refs, direct=rule in ("size", "diameter"), bounds_out=bounds)
        tie_tasks = sum(r["tie"] for r in refs)
        print(f"split_cut {rule} d={d} {cls}: value {verdict['value']:.3f} mean {verdict['mean']:.3f} of the bound, undecided "
              f"{share:.3f}, tie tasks {out['ties']}, generic {int(out['route'].sum())}")
        assert sc.passes(verdict), (rule, verdict)
        assert out["ties"] == tie_tasks, (rule, out["ties"], tie_tasks)
        if rule == "rss":
            assert [int(r) for r in out["route"]] == [_expected_route(z, off, t) for t in range(T)]
            hom = [t for t in range(T) if z[off[t]:off[t + 1]].min() == z[off[t]:off[t + 1]].max()]
            assert hom and all(out["rc"][t] == sc.E_HOMOGENEOUS for t in hom)
            assert all(out["rc"][t] == sc.OK for t in range(T) if t not in hom)
            for t in range(T):  # the seeds: the FIRST row of the least and of the greatest projection
                if out["rc"][t] == sc.OK:
                    zt, kids = z[off[t]:off[t + 1]], out["children"][off[t]:off[t + 1]]
                    assert kids[0] == ids[off[t] + int(np.argmin(zt))] and kids[out["nlow"][t]] == ids[off[t] + int(np.argmax(zt))], t
        else:
            assert not out["route"].any()
        if rule in ("rss2", "size", "diameter"):
            assert all(out["rc"][t] == refs[t]["rc"] for t in range(T) if refs[t]["margin"] > 1.0)

        assert not _same(out, ctx.group_cut_test(ids, off, code, z), off), rule  # a second call: the same bits
        for t in [t for t in range(T) if off[t + 1] - off[t] in ALONE_LENS]:  # alone in its batch: the same bits
            o1 = np.array([0, off[t + 1] - off[t]], dtype=np.int32)
            one = ctx.group_cut_test(ids[off[t]:off[t + 1]], o1, code, z[off[t]:off[t + 1]])
            inside = {k: out[k][t:t + 1] for k in BITS if k != "children"}
            inside.update(children=out["children"][off[t]:off[t + 1]], ties=int(refs[t]["tie"]))
            assert not _same(one, inside, o1), (rule, t)

        if rule == "rss":  # form against form: every task by the generic host path
            gen = ctx.group_cut_test(ids, off, code, z, force_generic=True)
            vg = sc.judge(X, w, ids, off, gen, refs)
            print(f"    generic path: value {vg['value']:.3f} mean {vg['mean']:.3f} of the bound")
            assert sc.passes(vg) and gen["route"].all(), vg
            assert np.array_equal(gen["rc"], out["rc"])
            for t in range(T):  # decided: the same children (both are the reference's), the values within the bound of each other
                if refs[t]["margin"] > 1.0 and out["rc"][t] == sc.OK:
                    assert np.array_equal(gen["children"][off[t]:off[t + 1]], out["children"][off[t]:off[t + 1]]), t
                    for q, key in enumerate(("vlow", "vhigh")):
                        assert abs(sc.LD(gen[key][t]) - sc.LD(out[key][t])) <= 2 * bounds[t, q], (t, key)
            for t in np.flatnonzero(out["route"] == 1):  # a declined task IS the generic path: the same bits
                assert gen["nlow"][t] == out["nlow"][t] and gen["vlow"][t] == out["vlow"][t] and gen["vhigh"][t] == out["vhigh"][t]
                assert np.array_equal(gen["children"][off[t]:off[t + 1]], out["children"][off[t]:off[t + 1]])
                assert np.array_equal(gen["cmeans"][t].view(np.int64), out["cmeans"][t].view(np.int64)), t


@pytest.mark.parametrize("d", [1, 5, 63, 64, 65, 128])
@pytest.mark.parametrize("cls", ["integer", "gaussian", "offset"])
def test_rss2_forms_give_the_same_bits(ctx, cells, cls, d):
    """chain + merge (d <= 128) against the one-kernel walk rss2_walk_kernel<1 | 2>"""
    X, w, ids, off, z, refs = cells("rss2", d, cls)
    ctx = _load(ctx, X, w)
    try:
        ctx.set_option("test_rss2_one_kernel", 0)
        a = ctx.group_cut_test(ids, off, sc.RSS2, z)
        ctx.set_option("test_rss2_one_kernel", 1)
        b = ctx.group_cut_test(ids, off, sc.RSS2, z)
    finally:
        ctx.set_option("test_rss2_one_kernel", 0)
    assert not _same(a, b, off)
    assert sc.passes(sc.judge(X, w, ids, off, b, refs))


@pytest.mark.parametrize("rule", RULE_NAMES)
def test_long_group_among_many_short_ones(ctx, cells, rule):
    """The third form of the per-group sort: a batch whose longest group exceeds the 8 LDS pieces (32769 rows) and whose groups
    are short on average (64 groups of 64 rows beside it: fewer than 768 rows a group) takes rocPRIM's SEGMENTED sort, where the
    cell's batch takes two device-wide sorts.  The long group: the same bits as inside the cell's batch; the short ones: judged
    against a reference of their own"""
    d, cls = 5, "gaussian"
    X, w, ids, off, z, refs = cells(rule, d, cls)
    ctx = _load(ctx, X, w)
    lens = np.diff(off)
    tl, ts = int(np.flatnonzero(lens == 32769)[0]), int(np.flatnonzero(lens == 4096)[0])
    order = np.concatenate([np.arange(off[ts], off[ts] + 2048), np.arange(off[tl], off[tl + 1]), np.arange(off[ts] + 2048, off[ts + 1])])
    sub_ids, sub_z = ids[order], z[order]
    sub_off = np.concatenate([np.arange(0, 2049, 64), 2048 + 32769 + np.arange(0, 2049, 64)]).astype(np.int32)
    T, at = len(sub_off) - 1, 32
    assert sub_off[at + 1] - sub_off[at] == 32769 and sub_off[-1] == len(order) and sub_off[-1] / T < 768
    code, direct = sc.RULES[rule], rule in ("size", "diameter")
    out = ctx.group_cut_test(sub_ids, sub_off, code, sub_z)
    cell = ctx.group_cut_test(ids, off, code, z)
    for key in ("rc", "nlow", "vlow", "vhigh", "route"):
        assert out[key][at] == cell[key][tl], key
    assert np.array_equal(out["cmeans"][at].view(np.int64), cell["cmeans"][tl].view(np.int64))
    if cell["rc"][tl] == sc.OK:
        assert np.array_equal(out["children"][sub_off[at]:sub_off[at + 1]], cell["children"][off[tl]:off[tl + 1]])
    short_refs = [refs[tl] if t == at else sc.split_group(X, w, sub_ids[sub_off[t]:sub_off[t + 1]], sub_z[sub_off[t]:sub_off[t + 1]], code)
                  for t in range(T)]
    verdict = sc.judge(X, w, sub_ids, sub_off, out, short_refs, direct=direct)
    assert sc.passes(verdict), verdict
    assert not _same(out, ctx.group_cut_test(sub_ids, sub_off, code, sub_z), sub_off)


@pytest.mark.parametrize("d", [5, 129])
@pytest.mark.parametrize("rule", RULE_NAMES)
def test_without_projections_the_whole_split_runs(ctx, cells, rule, d):
    """z == NULL: the statistics stage runs first.  Its projections are the ones cge_group_stats_test returns, and the result is
    the one of the supplied-z call fed with them, bit for bit: the new function boundary against the old single function"""
    X, w, ids, off = cells(rule, d, "separated")[:4]
    ctx = _load(ctx, X, w)
    whole = ctx.group_cut_test(ids, off, sc.RULES[rule], None)
    zdev = ctx.group_stats_test(ids, off)["z"]
    fed = ctx.group_cut_test(ids, off, sc.RULES[rule], zdev)
    assert not _same(whole, fed, off)
    refs = sc.reference_batch(X, w, ids, off, zdev, sc.RULES[rule])
    verdict = sc.judge(X, w, ids, off, whole, refs, direct=rule in ("size", "diameter"))
    print(f"split_cut {rule} d={d} separated, device projections: value {verdict['value']:.3f} mean {verdict['mean']:.3f}, "
          f"undecided {len(verdict['undecided'])}")
    assert sc.passes(verdict) and (whole["rc"] == sc.OK).all(), verdict


@pytest.mark.parametrize("rule", ["size", "diameter"])
def test_a_nan_projection_fails_its_task_alone(ctx, cells, rule):
    """A NaN among a group's projections makes the reference's median / mid-range NaN: every row goes high, the low child is empty
    and the split fails with CGE_E_EMPTY_CLUSTER.  (The sort puts NaNs at the two ends, by sign, so the middle of the sorted
    array is finite, and fmin / fmax skip a NaN: cut_sides_kernel propagates it by hand.)  The neighbours are untouched."""
    d, cls = 5, "gaussian"
    X, w, ids, off, z, _ = cells(rule, d, cls)
    ctx = _load(ctx, X, w)
    lens = np.diff(off)
    pick = [int(np.flatnonzero(lens == k)[0]) for k in (1025, 5, 64, 257, 4097, 17, 1033)]
    sub_ids = np.concatenate([ids[off[t]:off[t + 1]] for t in pick])
    sub_z = np.concatenate([z[off[t]:off[t + 1]] for t in pick])
    sub_off = np.concatenate([[0], np.cumsum(lens[pick])]).astype(np.int32)
    clean = ctx.group_cut_test(sub_ids, sub_off, sc.RULES[rule], sub_z)
    zn = sub_z.copy()
    zn[sub_off[1] + 2] = np.nan                       # 5 rows: one NaN
    zn[sub_off[3] + 256] = np.copysign(np.nan, -1.0)  # 257 rows: a NaN with the sign bit (sorts first), in the last row
    zn[sub_off[4] + 7], zn[sub_off[4] + 4096] = np.nan, np.copysign(np.nan, -1.0)  # 4097 rows: both kinds, two sorted pieces
    bad = (1, 3, 4)
    refs = sc.reference_batch(X, w, sub_ids, sub_off, zn, sc.RULES[rule])
    assert [r["rc"] for r in refs] == [sc.E_EMPTY_CLUSTER if t in bad else sc.OK for t in range(len(pick))]
    out = ctx.group_cut_test(sub_ids, sub_off, sc.RULES[rule], zn)
    assert sc.passes(sc.judge(X, w, sub_ids, sub_off, out, refs, direct=True))
    assert [int(r) for r in out["rc"]] == [r["rc"] for r in refs] and all(out["nlow"][t] == 0 for t in bad)
    keep = [t for t in range(len(pick)) if t not in bad]
    for k in ("rc", "nlow", "vlow", "vhigh", "cmeans"):
        assert np.array_equal(out[k][keep], clean[k][keep]), k
    for t in keep:
        assert np.array_equal(out["children"][sub_off[t]:sub_off[t + 1]], clean["children"][sub_off[t]:sub_off[t + 1]])


@pytest.mark.parametrize("force_generic", [0, 1])
def test_a_nan_projection_under_rss_is_a_homogeneous_group(ctx, cells, force_generic):
    """The reference's argmin and argmax both return the FIRST NaN of z, so l1 == l2 and split_cluster_rss throws "Trying to split
    homogenous cluster" (src/landmarks.jl:163-166).  The sorted form declines a group with a NaN, and the generic host path refuses
    it before its arg-min / arg-max scan (whose comparisons skip a NaN) and its median (std::nth_element is undefined on one): a NaN
    in the first row, in the middle, and in place of the group's maximum.  The neighbours are untouched, bit for bit."""
    d, cls = 5, "gaussian"
    X, w, ids, off = cells("rss", d, cls)[:4]
    ctx = _load(ctx, X, w)
    lens = np.diff(off)
    pick = [int(np.flatnonzero(lens == k)[0]) for k in (1025, 5, 64, 257, 4097, 17, 3, 1033)]
    sub_ids = np.concatenate([ids[off[t]:off[t + 1]] for t in pick])
    sub_z = np.random.default_rng(17).standard_normal(len(sub_ids))  # distinct: every group splits, none by the generic path
    sub_off = np.concatenate([[0], np.cumsum(lens[pick])]).astype(np.int32)
    clean = ctx.group_cut_test(sub_ids, sub_off, sc.RSS, sub_z, force_generic=bool(force_generic))
    assert (clean["rc"] == sc.OK).all()
    zn = sub_z.copy()
    zn[sub_off[1]] = np.nan                                                   # 5 rows: the first row
    zn[sub_off[3] + 128] = np.copysign(np.nan, -1.0)                          # 257 rows: the middle, a NaN with the sign bit
    zn[sub_off[4] + int(np.argmax(sub_z[sub_off[4]:sub_off[5]]))] = np.nan    # 4097 rows (two sorted pieces): the maximum
    zn[sub_off[6] + 1] = np.nan                                               # 3 rows: the middle of the shortest group
    bad = (1, 3, 4, 6)
    out = ctx.group_cut_test(sub_ids, sub_off, sc.RSS, zn, force_generic=bool(force_generic))
    assert [int(r) for r in out["rc"]] == [sc.E_HOMOGENEOUS if t in bad else sc.OK for t in range(len(pick))]
    assert all(out["route"][t] == 1 for t in bad)  # whichever form was asked for, the generic path booked them
    keep = [t for t in range(len(pick)) if t not in bad]
    for k in ("rc", "nlow", "vlow", "vhigh", "cmeans", "route"):
        assert np.array_equal(_bits_of(out[k][keep]), _bits_of(clean[k][keep])), k
    for t in keep:
        assert np.array_equal(out["children"][sub_off[t]:sub_off[t + 1]], clean["children"][sub_off[t]:sub_off[t + 1]])
    assert not _same(out, ctx.group_cut_test(sub_ids, sub_off, sc.RSS, zn, force_generic=bool(force_generic)), sub_off)


def _bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def test_group_cut_hook_refusals(ctx, cells):
    from cge.jl_amd import api

    get = ctx
    X, w, ids, off = cells("rss", 5, "integer")[:4]
    ctx = _load(get, X, w)
    z3, o3 = np.array([1.0, 2.0, 3.0]), np.array([0, 3], dtype=np.int32)
    with pytest.raises(api.CGEError, match="fewer than 3"):
        ctx.group_cut_test(ids[:5], np.array([0, 3, 5], dtype=np.int32), sc.RSS, np.arange(5.0))
    with pytest.raises(api.CGEError, match="outside"):
        ctx.group_cut_test(np.array([1, 2, len(w)], dtype=np.int32), o3, sc.SIZE, z3)
    with pytest.raises(api.CGEError, match="two groups"):
        ctx.group_cut_test(np.array([4, 7, 4], dtype=np.int32), o3, sc.SIZE, z3)
    with pytest.raises(api.CGEError, match="unknown method"):
        ctx.group_cut_test(ids[:3], o3, 4, z3)
    out = ctx.group_cut_test(ids[:3], o3, sc.DIAMETER, z3)  # (the context still works after a refusal)
    assert out["rc"][0] == sc.OK and out["nlow"][0] == 1 and out["ties"] == 1
    X, w, ids, off = sc.make_problem("integer", 513)
    ctx = get(len(w) + 1)  # (a context of its own: d = 513 and its row count differ from every cell's)
    ctx.set_vertex_data(np.ones(len(w), dtype=np.int64), w)
    ctx.set_embedding(X)
    z = sc.make_projections("integer", 513, sc.SIZE, off)
    for code in (sc.RSS, sc.RSS2):
        with pytest.raises(api.CGEError, match="512") as e:
            ctx.group_cut_test(ids, off, code, z)
        assert e.value.code == sc.E_ARG
