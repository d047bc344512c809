"""CPU tests of tests/louvain_levels_ref.py, the numpy restatement of the Louvain hierarchy (contraction + the level rule
around `louvain_ref.sync_level1`).  The GPU tests (test_gpu_louvain_levels.py) then hold the device to it."""
import numpy as np
import pytest

import louvain_graphs as lg
import louvain_levels_ref as ll
from louvain_ref import modularity, sync_level1

KNOWN = ll.known_answers()


@pytest.mark.parametrize("name", list(KNOWN))
def test_levels_known_answers_and_their_invariants(name):
    e, w, n, counts = KNOWN[name]
    graphs = []
    lv = ll.levels(e, w, n, graphs=graphs)
    print(name, [(nc, q, r) for _, nc, q, r in lv])
    assert [nc for _, nc, _, _ in lv] == counts
    for l, (comm, nc, q, rounds) in enumerate(lv):
        assert comm.shape == (n,) and comm.min() == 0 and comm.max() == nc - 1 and len(np.unique(comm)) == nc
        # the modularity a level reports is that of the composed partition on the ORIGINAL graph, bit for bit
        assert q == modularity(e, w, n, comm)
        if l:
            prev = lv[l - 1]
            assert nc < prev[1]  # strictly decreasing
            # every level refines to the next: a community of level l lies in one community of level l + 1
            assert len(np.unique(prev[0] * nc + comm)) == prev[1]
    # the dropped level is the first that merges nothing: a pass on the contraction of the last reported level
    ge, gw, gn, gcomm = graphs[-1]
    last_nc = lv[-1][1]
    if last_nc < gn:
        ce, cw = ll.contract(ge, gw, gn, gcomm, last_nc)
        assert sync_level1(ce, cw, last_nc)[1] == last_nc
    else:
        assert len(lv) == 1  # level 1 merged nothing and is reported all the same


def test_contraction_keeps_degrees_total_weight_and_modularity():
    rng = np.random.default_rng(3)
    for n in (9, 40, 65, 300):
        e, _ = lg.random_multigraph(n, seed=n)
        for w in (None, rng.integers(1, 17, size=len(e)) / 4.0):
            comm, nc, q, _ = sync_level1(e, w, n)
            ce, cw = ll.contract(e, w, n, comm, nc)
            assert len(np.unique(np.sort(ce, axis=1), axis=0)) == len(ce)  # repeated edges are merged
            ww = np.ones(len(e)) if w is None else w
            k = np.zeros(n)
            np.add.at(k, e[:, 0], ww)
            np.add.at(k, e[e[:, 0] != e[:, 1], 1], ww[e[:, 0] != e[:, 1]])
            kc = np.zeros(nc)
            np.add.at(kc, ce[:, 0], cw)
            np.add.at(kc, ce[ce[:, 0] != ce[:, 1], 1], cw[ce[:, 0] != ce[:, 1]])
            assert np.array_equal(kc, np.bincount(comm, weights=k, minlength=nc))  # k_C = tot_C, so m2 is unchanged
            assert modularity(ce, cw, nc, np.arange(nc)) == q  # the coarse singletons = the fine partition


def test_max_levels_and_a_graph_of_self_loops():
    e, w, n, counts = KNOWN["chain257x3"]
    full = ll.levels(e, w, n)
    for k in (1, 2, 3, 9):
        part = ll.levels(e, w, n, max_levels=k)
        assert len(part) == min(k, len(counts))
        for a, b in zip(part, full):
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    lv = ll.levels(np.array([[0, 0], [2, 2], [2, 2], [4, 4]]), None, 5)
    assert len(lv) == 1 and lv[0][1] == 5 and lv[0][3] == 0 and lv[0][0].tolist() == [0, 1, 2, 3, 4]


def test_hub_and_pairs_has_one_long_segment_at_level_two():
    """The graph of the wave form's GPU test: level 1 finds the triangles, level 2 pairs them."""
    for P, counts, longest in ((40, None, 17), (200, None, 57), (1100, [2200, 1097], 282)):
        e, n = ll.hub_and_pairs(P)
        assert n == 8 + 6 * P and len(e) == 28 + 10 * P
        graphs = []
        lv = ll.levels(e, None, n, graphs=graphs)
        print(P, [nc for _, nc, _, _ in lv], [ll.longest_segment(g[0], g[2]) for g in graphs])
        if counts:
            assert [nc for _, nc, _, _ in lv] == counts
        assert len(graphs) >= 2 and ll.longest_segment(graphs[1][0], graphs[1][2]) == longest
