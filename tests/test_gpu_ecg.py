"""ECG on the device (`cge_ecg`, csrc/kernels_louvain.hip) against its numpy restatement tests/ecg_ref.py: the members in rank
space, the lock-step groups, the 2-core, the weights, the hierarchy on them, the two modularities, the interface.

Compared to the bit: unit and `louvain_levels_ref.dyadic` weights with K = 8 members and w_min = 1/8, so that every ECG weight is a
multiple of 1/64 and every sum is exact in any order.  `weighted_clique_ring` (1.3 / 0.7 / ...) is compared in quality alone.

By the definition (all vertices with fewer than 2 live entries go together, round after round) the 257-vertex path takes 129
rounds that remove something: 128 take its two ends, and the middle vertex goes alone in the last one.  The device is held to the
restatement's count, and that count is pinned here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ecg_ref
import louvain_graphs as lg
import louvain_levels_ref as ll
from conftest import ROOT
from louvain_ref import modularity

pytestmark = pytest.mark.gpu

CGE_E_ARG = -7
K, W_MIN, SEED = 8, 0.125, 3
RANDOM = {63: 1, 64: 2, 65: 3, 255: 1, 256: 3, 257: 2, 1025: 3}  # n -> seed of random_multigraph
CORES = {63: 59, 257: 233, 1025: 928}


def cycle_with_tail(cycle=24, tail=40):
    e, _ = lg.cycle(cycle)
    t = [(0, cycle)] + [(cycle + i, cycle + i + 1) for i in range(tail - 1)]
    return np.concatenate([e, np.asarray(t, dtype=np.int64)]), cycle + tail


def _cases():
    cases = {}
    for n, seed in RANDOM.items():
        e, _ = lg.random_multigraph(n, seed=seed)  # self loops, repeated edges, isolated vertices
        cases[f"random{n}"] = (e, None, n)
        cases[f"random{n}_dyadic"] = (e, ll.dyadic(e, 100 * n + seed), n)
    for name, (e, n) in {"path257": lg.path(257), "star65": lg.star(65), "ring16x5": lg.clique_chain(16, 5, ring=True),
                         "barbell6_3": lg.barbell(6, 3), "cycle24_tail40": cycle_with_tail()}.items():
        cases[name] = (e, None, n)
        cases[name + "_dyadic"] = (e, ll.dyadic(e, len(e)), n)
    return cases


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _ref(name, members=K, w_min=W_MIN, final_level=-1):
    e, w, n = CASES[name]
    return ecg_ref.ecg(e, w, n, members, w_min, SEED, final_level)


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.set_option("ecg_group", 0)
    c.close()


def _upload(ctx, e, w, n):
    ctx.set_graph(np.asarray(e) + 1, np.ones(len(e)) if w is None else w, n)


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def _same_result(dev, ref):
    comm, nc, q, q_ecg, weights = dev
    assert nc == ref["n_comm"] and np.array_equal(comm, ref["comm"]), (nc, ref["n_comm"])
    assert _bits(q) == _bits(ref["q"]) and _bits(q_ecg) == _bits(ref["q_ecg"]), (q, ref["q"], q_ecg, ref["q_ecg"])
    assert _bits(weights) == _bits(ref["weights"])


def _same_members(dev, ref):
    mem, nc, rounds, q, core = dev
    assert np.array_equal(mem, ref["members"])
    assert list(nc) == ref["member_nc"] and list(rounds) == ref["member_rounds"], (list(rounds), ref["member_rounds"])
    assert _bits(q) == _bits(ref["member_q"]), (q, ref["member_q"])
    assert np.array_equal(core, ref["core"])


@pytest.mark.parametrize("name", list(CASES))
def test_members_core_weights_partition_and_modularities_equal_the_restatement(ctx, name):
    e, w, n = CASES[name]
    ref = _ref(name)
    _upload(ctx, e, w, n)
    ctx.set_option("ecg_group", 0)
    members = ctx.ecg_members_test(K, SEED)
    print(name, "members", list(members[1]), list(members[2]), "core", int(members[4].sum()), "peel", ctx.get_stat("ecg_peel_rounds"),
          "restatement", ref["member_nc"], ref["member_rounds"], int(ref["core"].sum()), ref["peel_rounds"])
    _same_members(members, ref)
    assert ctx.get_stat("ecg_peel_rounds") == ref["peel_rounds"]
    assert ctx.get_stat("ecg_member_rounds") == sum(ref["member_rounds"])
    dev = ctx.ecg(K, W_MIN, SEED, edge_weights=True)
    print(name, "device", dev[1:4], "restatement", ref["n_comm"], ref["q"], ref["q_ecg"], ref["levels"])
    _same_result(dev, ref)
    assert ctx.get_stat("ecg_levels") == ref["levels"] and ctx.get_stat("ecg_peel_rounds") == ref["peel_rounds"]
    comm = dev[0]
    assert comm.min() == 0 and comm.max() == dev[1] - 1 and len(np.unique(comm)) == dev[1]
    assert dev[2] == modularity(e, w, n, comm) and dev[3] == modularity(e, dev[4], n, comm)
    assert dev[4].min() >= W_MIN and dev[4].max() <= 1.0
    off_core = ~(ref["core"][e[:, 0]] & ref["core"][e[:, 1]])
    assert np.all(dev[4][off_core] == W_MIN)
    plain = ctx.ecg(K, W_MIN, SEED)  # no weights asked for: the same partition and scalars
    assert len(plain) == 4 and np.array_equal(plain[0], comm) and plain[1:] == dev[1:4]


def test_what_the_graphs_are_there_for():
    for n, core in CORES.items():
        ref = _ref(f"random{n}")
        assert int(ref["core"].sum()) == core
        assert len({m.tobytes() for m in ref["members"]}) >= 2  # relabelling alone gives the members variety
    assert _ref("path257")["core"].sum() == 0 and _ref("path257")["peel_rounds"] == 129
    assert _ref("star65")["n_comm"] == 1 and _ref("star65")["core"].sum() == 0
    ring = _ref("ring16x5")
    assert ring["n_comm"] == 16 and np.array_equal(ring["comm"], lg.clique_labels(16, 5))
    tail = _ref("cycle24_tail40")
    assert np.array_equal(np.flatnonzero(tail["core"]), np.arange(24)) and tail["peel_rounds"] == 40


@pytest.mark.parametrize("name", ["random63", "random257_dyadic", "random1025", "path257", "ring16x5_dyadic"])
def test_results_do_not_depend_on_the_group_size(ctx, name):
    """ecg_group = 1 (one member at a time), 3 (3 + 3 + 2: a ragged last group) and 0 (all eight together)."""
    e, w, n = CASES[name]
    ref = _ref(name)
    _upload(ctx, e, w, n)
    try:
        for group, groups in ((1, 8), (3, 3), (0, 1)):
            ctx.set_option("ecg_group", group)
            _same_members(ctx.ecg_members_test(K, SEED), ref)
            assert ctx.get_stat("ecg_groups") == groups
            _same_result(ctx.ecg(K, W_MIN, SEED, edge_weights=True), ref)
            assert ctx.get_stat("ecg_groups") == groups
    finally:
        ctx.set_option("ecg_group", 0)


@pytest.mark.parametrize("name", ["random257", "random1025_dyadic", "barbell6_3"])
def test_calls_repeat_and_leave_cge_louvain_alone(ctx, name):
    e, w, n = CASES[name]
    ref = _ref(name)
    _upload(ctx, e, w, n)
    before = ctx.louvain()
    levels = ctx.louvain_levels()
    _same_result(ctx.ecg(K, W_MIN, SEED, edge_weights=True), ref)
    _same_result(ctx.ecg(K, W_MIN, SEED, edge_weights=True), ref)  # two calls in a row
    after = ctx.louvain()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    again = ctx.louvain_levels()
    assert len(levels) == len(again) and all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(levels, again))
    _same_result(ctx.ecg(K, W_MIN, SEED, edge_weights=True), ref)


def test_another_seed_gives_other_members_and_the_seed_is_a_bit_pattern(ctx):
    e, w, n = CASES["random257"]
    _upload(ctx, e, w, n)
    for seed in (0, -1, 2**62 + 5):
        ref = ecg_ref.ecg(e, w, n, 4, 0.25, seed)
        _same_members(ctx.ecg_members_test(4, seed), ref)
        _same_result(ctx.ecg(4, 0.25, seed, edge_weights=True), ref)
    assert not np.array_equal(ecg_ref.ecg(e, w, n, 4, 0.25, 0)["members"], ecg_ref.ecg(e, w, n, 4, 0.25, -1)["members"])


def test_one_member_sixty_four_members_and_the_level_asked_for(ctx):
    e, w, n = CASES["random257"]
    _upload(ctx, e, w, n)
    one = ctx.ecg(1, W_MIN, SEED, edge_weights=True)
    _same_result(one, _ref("random257", members=1))
    assert set(np.unique(one[4])) <= {W_MIN, 1.0}  # co-clustered by the one member or not
    _same_result(ctx.ecg(64, 0.25, SEED, edge_weights=True), _ref("random257", members=64, w_min=0.25))
    assert ctx.get_stat("ecg_member_rounds") == sum(_ref("random257", members=64, w_min=0.25)["member_rounds"])
    last, first = _ref("random257"), _ref("random257", final_level=1)
    assert last["levels"] >= 2 and first["levels"] == 1 and first["n_comm"] > last["n_comm"]
    _same_result(ctx.ecg(K, W_MIN, SEED, final_level=1, edge_weights=True), first)
    assert ctx.get_stat("ecg_levels") == 1
    _same_result(ctx.ecg(K, W_MIN, SEED, final_level=-1, edge_weights=True), last)
    _same_result(ctx.ecg(K, W_MIN, SEED, final_level=99, edge_weights=True), last)  # beyond the hierarchy: its last level
    zero = ctx.ecg(K, 0.0, SEED, edge_weights=True)  # w_min = 0: edges off the core weigh nothing
    _same_result(zero, _ref("random257", w_min=0.0))


def test_real_weights_are_comparable_in_quality(ctx):
    """1.3 / 0.7 / 0.5 / 0.9 / 0.4 / 1.1: the members' sums may round differently from run to run, so the partition is checked
    to be one and both modularities against the direct formula.  1e-12: fewer than 10^3 terms of order 1 in any order."""
    e, w, n, labels = lg.weighted_clique_ring(30, 5)
    _upload(ctx, e, w, n)
    comm, nc, q, q_ecg, weights = ctx.ecg(16, 0.05, 42, edge_weights=True)
    print(nc, q, q_ecg)
    assert comm.shape == (n,) and comm.min() == 0 and comm.max() == nc - 1 and len(np.unique(comm)) == nc
    assert weights.min() >= 0.05 and weights.max() <= 1.0
    assert q == pytest.approx(modularity(e, w, n, comm), abs=1e-12)
    assert q_ecg == pytest.approx(modularity(e, weights, n, comm), abs=1e-12)
    assert len(np.unique(labels[:150] * n + comm[:150])) == len(np.unique(comm[:150]))  # no community cuts a clique


def test_refusals_on_the_device(ctx):
    from cge.jl_amd import api

    fresh = api.Context(0)  # no resident graph
    try:
        with pytest.raises(api.CGEError) as err:
            fresh.ecg()
        assert err.value.code == CGE_E_ARG and "no resident graph" in str(err.value)
        with pytest.raises(api.CGEError) as err:
            fresh.ecg_members_test(4, 0)
        assert err.value.code == CGE_E_ARG and "no resident graph" in str(err.value)
    finally:
        fresh.close()
    e, w, n = CASES["random63"]
    _upload(ctx, e, w, n)
    for kw, word in ((dict(members=0), "members"), (dict(members=65), "members"), (dict(w_min=1.0), "w_min"),
                     (dict(w_min=-0.1), "w_min"), (dict(w_min=float("nan")), "w_min"), (dict(final_level=0), "final_level"),
                     (dict(final_level=-2), "final_level")):
        with pytest.raises(api.CGEError) as err:
            ctx.ecg(**kw)
        assert err.value.code == CGE_E_ARG and word in str(err.value), kw
    with pytest.raises(api.CGEError):
        ctx.set_option("ecg_group", 65)
    _same_result(ctx.ecg(K, W_MIN, SEED, edge_weights=True), _ref("random63"))  # a refusal leaves the context usable


def _vector(text):
    return [float(x) for x in text.strip().strip("[]").split(",")]


def test_command_line_ecg_writes_the_file_and_scores_on_it(ctx, tmp_path, capsys):
    """`--ecg 8 --seed 3` on the reference's 115-vertex fixture, in a process of its own: the .ecg file holds `Context.ecg` of that
    graph, and `-c` on that file gives the same vector (1e-9: the same communities, sums in another order at the most).

    The process runs with `--ecg-wmin 0.125`.  With the default 0.05 the ECG weights are not dyadic, the final hierarchy's sums
    round by the order of the float atomics, and a tie may break another way from call to call, as `cge_louvain` on real weights
    already may: 12 calls of `Context.ecg(8, 0.05, 3)` on this graph gave 2 to 3 distinct label vectors (always 12 communities and
    modularity 0.6005165407471079; the reweighted graph's 0.878451215758882 or ...8821), so a file and a second call cannot be held
    equal there.  At 1/8 every weight is a multiple of 1/64 and the file is determined to the bit.  The default floor is run too,
    in this process, for what holds at any weights: a valid file, and the same vector from `-c` on it."""
    import shutil

    import cge_cli

    g = os.path.join(ROOT, "tests", "golden", "test115")
    edge_file = str(tmp_path / "test.edgelist")
    shutil.copy(os.path.join(g, "test.edgelist"), edge_file)
    emb_file = os.path.join(g, "test_n2v.embedding")
    common = ["-g", edge_file, "-e", emb_file, "--seed", "3"]
    edges = np.loadtxt(edge_file, dtype=np.int64)[:, :2]
    base = int(edges.min())  # the fixture's ids start at 0; the file keeps the edge list's base
    n = int(edges.max()) + 1 - base
    assert n == 115

    def with_c(name):
        shutil.copy(edge_file + ".ecg", tmp_path / name)
        capsys.readouterr()
        assert cge_cli.main(common + ["-c", str(tmp_path / name)]) == 0
        return _vector(capsys.readouterr().out)

    r = subprocess.run([sys.executable, os.path.join(ROOT, "cge_cli.py")] + common + ["--ecg", "8", "--ecg-wmin", "0.125"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = _vector(r.stdout)
    tab = np.loadtxt(edge_file + ".ecg", dtype=np.int64)
    ctx.set_graph(edges + 1 - base, np.ones(len(edges)), n)
    comm, nc, _, _ = ctx.ecg(8, 0.125, 3)
    assert np.array_equal(tab[:, 0], np.arange(n) + base) and np.array_equal(tab[:, 1], comm) and 1 < nc < n
    assert np.array_equal(comm, ecg_ref.ecg(edges - base, None, n, 8, 0.125, 3)["comm"])
    assert len(vec) == 7 and all(np.isfinite(vec)) and vec == pytest.approx(with_c("dyadic.ecg"), rel=1e-9, abs=1e-12)
    os.remove(edge_file + ".ecg")
    capsys.readouterr()
    assert cge_cli.main(common + ["--ecg", "8"]) == 0  # the default floor, 0.05
    vec = _vector(capsys.readouterr().out)
    tab = np.loadtxt(edge_file + ".ecg", dtype=np.int64)
    assert np.array_equal(tab[:, 0], np.arange(n) + base)
    assert tab[:, 1].min() == 0 and len(np.unique(tab[:, 1])) == tab[:, 1].max() + 1 and 1 < tab[:, 1].max() + 1 < n
    assert len(vec) == 7 and all(np.isfinite(vec)) and vec == pytest.approx(with_c("default.ecg"), rel=1e-9, abs=1e-12)
