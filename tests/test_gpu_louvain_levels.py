"""The Louvain hierarchy on the device (`cge_louvain_levels`, csrc/kernels_louvain.hip) against its numpy restatement
tests/louvain_levels_ref.py: contraction, composition, the level rule, the wave form of the decision, the interface.

Every graph compared to the bit has integer or dyadic weights: there every sum is exact in any order, so partitions,
community counts, round counts and modularities of every level are determined.  `weighted_clique_ring` carries 1.3 / 0.7 /
0.9 / 0.4 / 1.1; it is compared to the bit with those rounded to quarters (1.25 / 0.75 / 1.0 / 0.5 / 1.0 -- the same edges,
repeated edge, self loops and isolated vertex), and as it stands by quality alone."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import louvain_graphs as lg
import louvain_levels_ref as ll
from conftest import ROOT
from louvain_ref import modularity

pytestmark = pytest.mark.gpu

CGE_E_ARG = -7
LANE_ONLY = 2**31 - 1


def _quarters(g):
    e, w, n, _ = g
    return e, np.round(w * 4.0) / 4.0, n


def _cases():
    cases = {k: v[:3] for k, v in ll.known_answers().items()}
    for n in (63, 64, 65, 255, 257, 1025):
        for seed in (1, 2, 3):
            e, _ = lg.random_multigraph(n, seed=seed)  # self loops, repeated edges, isolated vertices
            cases[f"random{n}_s{seed}"] = (e, None, n)
            cases[f"random{n}_s{seed}_dyadic"] = (e, ll.dyadic(e, 100 * n + seed), n)
    cases["weighted_ring8x5_quarters"] = _quarters(lg.weighted_clique_ring(8, 5))
    cases["weighted_ring30x5_quarters"] = _quarters(lg.weighted_clique_ring(30, 5))
    cases["self_loop_only_vertex"] = (np.array([[0, 1], [1, 2], [0, 2], [3, 3], [4, 5], [2, 4]]), None, 7)
    cases["all_self_loops"] = (np.array([[0, 0], [2, 2], [2, 2], [4, 4]]), None, 5)
    return cases


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(levels, graphs) of the restatement, computed once and shared."""
    e, w, n = CASES[name]
    graphs = []
    lv = ll.levels(e, w, n, graphs=graphs)
    return lv, graphs


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _upload(ctx, e, w, n):
    ctx.set_graph(np.asarray(e) + 1, np.ones(len(e)) if w is None else w, n)


def _same(a, b):
    """Two lists of levels agree in partition, n_comm, modularity (bits) and rounds."""
    assert len(a) == len(b), ([x[1] for x in a], [x[1] for x in b])
    for (ca, na, qa, ra), (cb, nb, qb, rb) in zip(a, b):
        assert (na, ra) == (nb, rb) and np.array_equal(ca, cb), (na, nb, ra, rb)
        assert np.float64(qa).tobytes() == np.float64(qb).tobytes(), (qa, qb)


@pytest.mark.parametrize("name", list(CASES))
def test_every_level_equals_the_restatement_level_one_is_cge_louvain_and_calls_repeat(ctx, name):
    e, w, n = CASES[name]
    ref, _ = _ref(name)
    _upload(ctx, e, w, n)
    before = ctx.louvain()
    dev = ctx.louvain_levels()
    print(name, "device", [(nc, q, r) for _, nc, q, r in dev], "restatement", [(nc, q, r) for _, nc, q, r in ref])
    _same(dev, ref)
    for comm, nc, q, _ in dev:
        assert comm.min() == 0 and comm.max() == nc - 1 and len(np.unique(comm)) == nc
        assert q == modularity(e, w, n, comm)  # of the composed partition on the ORIGINAL graph
    _same(dev[:1], [before])  # row 0 and its scalars are cge_louvain's
    _same([ctx.louvain()], [before])  # ... which a levels call leaves as it was
    _same(ctx.louvain_levels(), dev)  # a second call gives the same bits


@pytest.mark.parametrize("name", list(CASES))
def test_a_level_is_a_pass_on_the_contracted_graph_device_against_device(ctx, name):
    """The restated contraction of level L's graph, self-loop edges included, uploaded as a graph of its own: level 1 of
    it (`cge_louvain`, the lane kernel on a CSR filled from an edge list) is level L + 1 of the hierarchy before
    composition, and the contraction of the last level merges nothing."""
    e, w, n = CASES[name]
    _, graphs = _ref(name)
    _upload(ctx, e, w, n)
    dev = ctx.louvain_levels()
    assert len(dev) == len(graphs)
    for l, (ge, gw, gn, gcomm) in enumerate(graphs):
        nc = dev[l][1]
        if nc == gn:
            assert l == 0 and len(dev) == 1  # level 1 merged nothing: the hierarchy ends there
            break
        ce, cw = ll.contract(ge, gw, gn, gcomm, nc)
        _upload(ctx, ce, cw, nc)
        comm, nc2, q2, rounds2 = ctx.louvain()
        if l + 1 < len(dev):
            un = np.zeros(nc, dtype=np.int64)
            un[dev[l][0]] = dev[l + 1][0]  # level l + 2 of the original vertices, per community of level l + 1
            _same([(comm, nc2, q2, rounds2)], [(un, dev[l + 1][1], dev[l + 1][2], dev[l + 1][3])])
        else:
            assert nc2 == nc  # the dropped level


@pytest.mark.parametrize("intra,bridge", [(1.3, 0.7), (0.7, 1.3)])
def test_real_weights_are_comparable_in_quality(ctx, intra, bridge):
    """1.3 / 0.7 (the cliques, one level) and 0.7 / 1.3 (the cliques, then pairs of them): sums may round differently from
    run to run, so structure and quality are checked, not the rounds.  1e-12: fewer than 10^3 terms of order 1 in any order."""
    e, w, n, labels = lg.weighted_clique_ring(30, 5, intra, bridge)
    _upload(ctx, e, w, n)
    dev = ctx.louvain_levels()
    print(intra, bridge, [(nc, q, r) for _, nc, q, r in dev])
    assert np.array_equal(dev[0][0], labels) and len(dev) == (1 if intra > bridge else 2)
    for l, (comm, nc, q, _) in enumerate(dev):
        assert q == pytest.approx(modularity(e, w, n, comm), abs=1e-12)
        if l:
            assert nc < dev[l - 1][1] and len(np.unique(dev[l - 1][0] * nc + comm)) == dev[l - 1][1]
            assert q > dev[l - 1][2]


@functools.lru_cache(maxsize=None)
def _hub(P):
    e, n = ll.hub_and_pairs(P)
    graphs = []
    return e, n, ll.levels(e, None, n, graphs=graphs), graphs


@pytest.mark.parametrize("P,longest", [(40, 17), (200, 57), (1100, 282)])
def test_wave_form_of_the_decision_agrees_with_the_lane_form(ctx, P, longest):
    """Hub and pairs: the level-2 graph has one long adjacency segment among short ones (17 and 57 entries: below and
    around one 64-entry chunk, so the chunk carry runs only when the form is forced; 282: four chunks and a rest, above
    the default length).  Default length, the wave form for every vertex, the wave form off: the same bits."""
    e, n, ref, graphs = _hub(P)
    assert ll.longest_segment(graphs[1][0], graphs[1][2]) == longest
    if P == 1100:
        assert [nc for _, nc, _, _ in ref] == [2200, 1097]
    _upload(ctx, e, None, n)
    try:
        for knob in (-2, -1, LANE_ONLY):
            ctx.set_option("louvain_wave_len", knob)
            dev = ctx.louvain_levels()
            print(P, knob, [(nc, q, r) for _, nc, q, r in dev])
            _same(dev, ref)
    finally:
        ctx.set_option("louvain_wave_len", -2)


@pytest.mark.parametrize("name", ["random1025_s1_dyadic", "chain257x3", "random300"])
def test_wave_form_forced_on_graphs_with_many_levels(ctx, name):
    e, w, n = CASES[name]
    ref, _ = _ref(name)
    _upload(ctx, e, w, n)
    try:
        ctx.set_option("louvain_wave_len", -1)
        _same(ctx.louvain_levels(), ref)
    finally:
        ctx.set_option("louvain_wave_len", -2)


def _raw(ctx, max_levels, cap, n):
    comm = np.full((max(cap, 1), n), -1, dtype=np.int64)
    nc, q, r = np.zeros(max(cap, 1), dtype=np.int64), np.zeros(max(cap, 1)), np.zeros(max(cap, 1), dtype=np.int64)
    count = C.c_int64(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx.L.cge_louvain_levels(ctx.h, C.c_int64(max_levels), C.c_int64(cap), p(comm) if cap else None, C.byref(count),
                                  p(nc) if cap else None, p(q) if cap else None, p(r) if cap else None)
    return rc, count.value, comm, nc, q, r


def test_interface_max_levels_count_only_and_refusals(ctx):
    from cge.jl_amd import api

    name = "chain257x3"  # 257 -> 122 -> 58 -> 31
    e, w, n = CASES[name]
    ref, _ = _ref(name)
    _upload(ctx, e, w, n)
    for k in (1, 2):
        _same(ctx.louvain_levels(max_levels=k), ref[:k])
    _same(ctx.louvain_levels(max_levels=9), ref)
    assert _raw(ctx, 0, 0, n)[:2] == (0, 4) and _raw(ctx, 2, 0, n)[:2] == (0, 2)  # levels_cap = 0: the count alone
    rc, count, comm, nc, q, r = _raw(ctx, 0, 4, n)
    assert (rc, count) == (0, 4)
    _same([(comm[l], int(nc[l]), float(q[l]), int(r[l])) for l in range(4)], ref)
    rc, count, comm, nc, _, _ = _raw(ctx, 0, 2, n)  # a cap that is too small
    assert (rc, count) == (CGE_E_ARG, 4) and "4 levels" in ctx.L.cge_last_error(ctx.h).decode()
    with pytest.raises(api.CGEError) as err:
        ctx._check(rc)
    assert err.value.code == CGE_E_ARG
    fresh = api.Context(0)  # no resident graph
    try:
        assert _raw(fresh, 0, 0, n)[0] == CGE_E_ARG and _raw(fresh, 0, 1, n)[0] == CGE_E_ARG
        assert "no resident graph" in fresh.L.cge_last_error(fresh.h).decode()
    finally:
        fresh.close()


def _ring_files(tmp_path):
    """A ring of 30 five-cliques (30 -> 16 communities) as a 1-based edge file, and an embedding that follows the cliques."""
    e, n = lg.clique_chain(30, 5, ring=True)
    edge_file = tmp_path / "ring.edgelist"
    np.savetxt(edge_file, e + 1, fmt="%d")
    rng = np.random.default_rng(5)
    ang = 2.0 * np.pi * lg.clique_labels(30, 5) / 30.0
    emb = np.stack([np.cos(ang), np.sin(ang), np.cos(2 * ang), np.sin(2 * ang)], axis=1) + 0.05 * rng.standard_normal((n, 4))
    emb_file = tmp_path / "ring.embedding"
    with open(emb_file, "w") as f:
        for i in range(n):
            f.write(f"{i + 1} " + " ".join(repr(float(x)) for x in emb[i]) + "\n")
    return e, n, str(edge_file), str(emb_file)


def test_louvain_clust_writes_the_level_asked_for(ctx, tmp_path):
    import cge.jl_amd as cg

    e, n, edge_file, _ = _ring_files(tmp_path)
    ref = ll.levels(e, None, n)
    assert [x[1] for x in ref] == [30, 16]
    for level, want in ((1, ref[0]), (2, ref[1]), (-1, ref[1]), (7, ref[1])):  # beyond the hierarchy: its last level
        out = cg.louvain_clust(1.0, edge_file, ctx=ctx, level=level) if level != 1 else cg.louvain_clust(1.0, edge_file, ctx=ctx)
        tab = np.loadtxt(out, dtype=np.int64)
        assert np.array_equal(tab[:, 0], np.arange(n) + 1) and np.array_equal(tab[:, 1], want[0]), level
    w = ll.dyadic(e, 9)
    refw = ll.levels(e, w, n)
    out = cg.louvain_clust(str(tmp_path / "ringw"), e + 1, w, ctx=ctx, level=-1)
    assert np.array_equal(np.loadtxt(out, dtype=np.int64)[:, 1], refw[-1][0])
    import inspect

    assert inspect.signature(cg.louvain_clust).parameters["level"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError):
        cg.louvain_clust(1.0, edge_file, ctx=ctx, level=0)


def _cli(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cge_cli.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [float(x) for x in r.stdout.strip().strip("[]").split(",")]


def test_command_line_without_c_scores_on_the_level_asked_for(tmp_path, capsys):
    """`--louvain-level 2` (an extension of this project's) in a process of its own: the .ecg holds level 2, and the vector
    is the one `-c` gives with those communities -- so the score ran on C = 16.  Without the flag: level 1 and today's
    vector.  The `-c` runs are in this process; 1e-9: the same communities, sums in another order at the most."""
    import cge_cli

    def with_c(comm, file):
        np.savetxt(file, np.stack([np.arange(n) + 1, comm], axis=1), fmt="%d")
        capsys.readouterr()
        assert cge_cli.main(common + ["-c", str(file)]) == 0
        return [float(x) for x in capsys.readouterr().out.strip().strip("[]").split(",")]

    e, n, edge_file, emb_file = _ring_files(tmp_path)
    ref = ll.levels(e, None, n)
    common = ["-g", edge_file, "-e", emb_file, "--seed", "3"]
    vec2 = _cli(common + ["--louvain-level", "2"])
    tab = np.loadtxt(edge_file + ".ecg", dtype=np.int64)
    assert np.array_equal(tab[:, 1], ref[1][0]) and len(np.unique(tab[:, 1])) == 16
    assert len(vec2) == 7 and all(np.isfinite(vec2))
    assert vec2 == pytest.approx(with_c(ref[1][0], tmp_path / "level2.ecg"), rel=1e-9, abs=1e-12)
    vec1 = _cli(common)  # no flag: level 1, as before
    tab = np.loadtxt(edge_file + ".ecg", dtype=np.int64)
    assert np.array_equal(tab[:, 1], ref[0][0]) and len(np.unique(tab[:, 1])) == 30
    assert vec1 == pytest.approx(with_c(ref[0][0], tmp_path / "level1.ecg"), rel=1e-9, abs=1e-12)
    assert vec1 != vec2
