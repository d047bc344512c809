"""CPU tests of tests/louvain_ref.py, the numpy restatement of the device's synchronous Louvain rounds, against the
oracle's sequential pass (`louvain_level1`: the published one_level(), nodes in natural order) and against graphs whose
communities are known.  The GPU tests (test_gpu_louvain.py) then hold the device to the restatement."""
import os

import numpy as np
import pytest

import louvain_graphs as lg
from conftest import GOLDEN, canonical_partition
from louvain_ref import modularity, sync_level1
from oracle import oracle as orc

FAMILIES = ([("path", lg.path(n)) for n in range(2, 25)] + [("cycle", lg.cycle(n)) for n in range(3, 41)] +
            [("star", lg.star(k)) for k in range(1, 11)] +
            [("ring", lg.clique_chain(c, s, ring=True)) for c in range(2, 12) for s in range(3, 7)] +
            [("chain", lg.clique_chain(c, s)) for c in range(2, 12) for s in range(3, 7)] +
            [("barbell", lg.barbell(a, p)) for a in range(3, 7) for p in range(6)])


def _fixture115():
    e = np.loadtxt(os.path.join(GOLDEN, "test115", "test.edgelist"), dtype=np.int64)[:, :2]
    return e, 115


def test_sync_rounds_are_as_good_as_the_sequential_pass_on_small_graphs():
    for name, (e, n) in FAMILIES:
        comm, nc, q, rounds = sync_level1(e, None, n)
        _, _, q_seq = orc.louvain_level1(e + 1, None, n)
        assert q >= q_seq - 1e-12, (name, n, q, q_seq)
        assert comm.min() == 0 and comm.max() == nc - 1 and len(np.unique(comm)) == nc and 1 <= rounds < 200
        assert modularity(e, None, n, comm) == pytest.approx(q, abs=1e-12), (name, n)


def test_cliques_are_recovered_exactly():
    for ring in (True, False):
        for c in range(2, 12):
            for s in range(3, 7):
                e, n = lg.clique_chain(c, s, ring=ring)
                comm, nc, _, _ = sync_level1(e, None, n)
                assert nc == c and np.array_equal(comm, lg.clique_labels(c, s)), (ring, c, s, comm)


def test_path5_goes_on_past_the_round_in_which_everyone_is_off_turn():
    """Rounds 1-2 give {0,1},{2},{3,4}; in round 3 vertex 2 wants to join {0,1} but is off turn and nothing else wants to
    move.  Stopping there leaves Q = 0.15625; the pass goes on and ends with {0,1,2},{3,4}, Q = 0.21875 = the oracle's."""
    e, n = lg.path(5)
    comm, nc, q, rounds = sync_level1(e, None, n)
    assert comm.tolist() == [0, 0, 0, 1, 1] and nc == 2 and rounds == 5
    assert q == 0.21875 == orc.louvain_level1(e + 1, None, n)[2]
    # two triangles joined through one middle vertex
    e, n = lg.barbell(3, 1)
    comm, nc, q, _ = sync_level1(e, None, n)
    assert q == pytest.approx(orc.louvain_level1(e + 1, None, n)[2], abs=1e-12) and q == pytest.approx(0.3672, abs=5e-5)
    assert nc == 2 and np.array_equal(canonical_partition(comm)[:6], [0, 0, 0, 1, 1, 1])


def test_reference_fixture():
    e, n = _fixture115()
    comm, nc, q, rounds = sync_level1(e, None, n)
    _, _, q_seq = orc.louvain_level1(e + 1, None, n)
    assert q >= q_seq - 0.03, (q, q_seq)  # the slack test_gpu_louvain.py gives the device against the sequential pass
    assert modularity(e, None, n, comm) == pytest.approx(q, abs=1e-12)


def test_self_loops_repeated_edges_and_isolated_vertices():
    # two vertices, one unit self loop each: the singletons have in = 2, tot = (1, 1), m2 = 2: Q = 1 - 2/4
    e = np.array([[0, 0], [1, 1]])
    comm, nc, q, rounds = sync_level1(e, None, 2)
    assert comm.tolist() == [0, 1] and nc == 2 and q == 0.5 and rounds == 0
    assert modularity(e, None, 2, comm) == 0.5 == orc.louvain_level1(e + 1, None, 2)[2]
    # the modularity formula against the oracle's bookkeeping, on the partitions the oracle itself returns
    rng = np.random.default_rng(7)
    for n in (2, 3, 9, 40, 65):
        e, _ = lg.random_multigraph(n, seed=n)
        for w in (None, rng.integers(1, 17, size=len(e)) / 4.0):
            c_seq, _, q_seq = orc.louvain_level1(e + 1, w, n)
            assert modularity(e, w, n, c_seq) == pytest.approx(q_seq, abs=1e-12)
            comm, nc, q, _ = sync_level1(e, w, n)
            assert modularity(e, w, n, comm) == pytest.approx(q, abs=1e-12)
            untouched = np.setdiff1d(np.arange(n), e.ravel())
            assert all((comm == comm[v]).sum() == 1 for v in untouched)  # an isolated vertex stays alone
