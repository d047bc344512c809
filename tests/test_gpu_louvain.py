"""`louvain_clust` (src/clustering.jl:14-68) on the device -- SURVEY section 8(f) rank 4.  The reference's executable
visits the vertices in an unseeded random order, so partitions are compared by quality: against the sequential
restatement in the oracle, against networkx, and against planted communities."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import louvain_graphs as lg
from conftest import GOLDEN, ROOT
from louvain_ref import modularity, sync_level1

pytestmark = pytest.mark.gpu
nx = pytest.importorskip("networkx")


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _nx_modularity(edges, n, comm, weights=None):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    if weights is None:
        G.add_edges_from((np.asarray(edges) - 1).tolist())
    else:
        G.add_weighted_edges_from([(int(u) - 1, int(v) - 1, float(w)) for (u, v), w in zip(np.asarray(edges), weights)])
    parts = [set(np.flatnonzero(comm == c).tolist()) for c in range(comm.max() + 1)]
    return nx.community.modularity(G, parts, weight="weight" if weights is not None else None)


def test_louvain_reference_fixture_and_planted_communities(ctx, test115):
    from cge.jl_amd import synth
    from oracle import oracle as orc

    n = len(test115["vweights"])
    cases = [(test115["edges"], None, n, None)]
    g = synth.abcd_like(20000, 200000, 20, 4, seed=1)
    cases.append((g["edges"], None, g["n"], g["comm"][:, 0]))
    rng = np.random.default_rng(4)
    g2 = synth.abcd_like(8000, 60000, 10, 4, seed=2)
    cases.append((g2["edges"], rng.integers(1, 9, size=g2["m"]) / 4.0, g2["n"], g2["comm"][:, 0]))
    for edges, w, nn, truth in cases:
        ctx.set_graph(edges, np.ones(len(edges)) if w is None else w, nn)
        comm, nc, q, rounds = ctx.louvain()
        assert comm.min() == 0 and comm.max() == nc - 1 and len(np.unique(comm)) == nc and 1 <= rounds < 200
        assert _nx_modularity(edges, nn, comm, w) == pytest.approx(q, abs=1e-9)  # the reported modularity is the partition's
        _, _, q_seq = orc.louvain_level1(edges, w, nn)
        assert q >= q_seq - 0.03, (q, q_seq)  # as good as the sequential pass of the published algorithm
        comm2, nc2, q2, _ = ctx.louvain()
        if w is None:
            assert np.array_equal(comm, comm2) and q == q2  # unit weights: deterministic
        if truth is not None:
            purity = sum(np.bincount(truth[comm == c]).max() for c in range(nc)) / nn
            assert purity > 0.98 and nc < nn / 20


def test_louvain_clust_writes_the_ecg_file_and_parseargs_uses_it(ctx, tmp_path):
    """test/runtests.jl:105-114 (`louvain_clust(0.0, "test.edgelist")`, `louvain_clust("testw.edgelist", edges, weights)`:
    the file exists) -- plus what the file must contain, and the command line WITHOUT -c end to end."""
    import cge.jl_amd as cg

    src = os.path.join(GOLDEN, "test115")
    for f in ("test.edgelist", "test_weights.edgelist", "test_n2v.embedding"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    out = cg.louvain_clust(0.0, str(tmp_path / "test.edgelist"), ctx=ctx)
    assert os.path.isfile(out) and out.endswith("test.edgelist.ecg")
    tab = np.loadtxt(out, dtype=np.int64)
    assert tab.shape == (115, 2) and np.array_equal(tab[:, 0], np.arange(115)) and tab[:, 1].min() == 0
    a = cg.parseargs(["-g", str(tmp_path / "test_weights.edgelist"), "-e", str(tmp_path / "test_n2v.embedding"), "-l", "20"],
                     exit_on_error=False)
    assert os.path.isfile(tmp_path / "test_weights.edgelist.ecg")
    edges, ew, vw, comm, clusters = a[:5]
    assert comm.shape == (115, 1) and comm.min() == 1 and sum(len(c) for c in clusters) == 115
    # the whole command line without -c (Louvain -> landmarks -> wGCL), in its own process
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cge_cli.py"), "-g", str(tmp_path / "test.edgelist"), "-e",
                        str(tmp_path / "test_n2v.embedding"), "-l", "20", "--seed", "3", "--samples-local", "500"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    vec = [float(x) for x in r.stdout.strip().strip("[]").split(",")]
    assert len(vec) == 7 and all(np.isfinite(vec)) and 0.25 <= vec[0] <= 10.0


# ---- the rounds themselves: the device against tests/louvain_ref.py (numpy, fp64, the same expressions) ---------------------
EXACT_CASES = {
    "path5": lg.path(5), "path24": lg.path(24), "cycle17": lg.cycle(17), "star7": lg.star(7),
    "ring6x4": lg.clique_chain(6, 4, ring=True), "chain5x5": lg.clique_chain(5, 5), "barbell5_3": lg.barbell(5, 3),
    "triangles_through_a_vertex": lg.barbell(3, 1),
    **{f"random{n}": lg.random_multigraph(n, seed=n) for n in (2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097)},
    "star_of_cliques5001": lg.star_of_cliques(1000, 5),
    "self_loop_only_vertex": (np.array([[0, 1], [1, 2], [0, 2], [3, 3], [4, 5], [2, 4]]), 7),
    "all_self_loops": (np.array([[0, 0], [1, 1]]), 2),
    "all_self_loops_repeated": (np.array([[0, 0], [2, 2], [2, 2], [4, 4]]), 5),
}


def _device(ctx, e, w, n):
    ctx.set_graph(e + 1, np.ones(len(e)) if w is None else w, n)
    return ctx.louvain()


@pytest.mark.parametrize("weights", ["unit", "dyadic"])
@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_device_rounds_equal_the_restatement(ctx, name, weights):
    """Integer and dyadic weights (multiples of 1/4 up to 4): every sum is exact in any order, so partition, number of
    communities and round count are equal and the modularity agrees to the last few bits."""
    e, n = EXACT_CASES[name]
    w = None if weights == "unit" else np.random.default_rng(len(e)).integers(1, 17, size=len(e)) / 4.0
    comm, nc, q, rounds = _device(ctx, e, w, n)
    r_comm, r_nc, r_q, r_rounds = sync_level1(e, w, n)
    print(name, weights, "device", nc, q, rounds, "restatement", r_nc, r_q, r_rounds)
    assert (nc, rounds) == (r_nc, r_rounds) and np.array_equal(comm, r_comm)
    assert q == pytest.approx(r_q, abs=1e-12)


@pytest.mark.parametrize("cliques,size", [(8, 5), (30, 5), (12, 7)])
def test_real_weights_find_the_cliques_and_report_their_modularity(ctx, cliques, size):
    """Weights 1.3 / 0.7: sums may round differently from the restatement's and from run to run (atomics), so the structure
    and the quality are checked, not the rounds.  1e-12: fewer than 10^3 terms of order 1, summed in any order."""
    e, w, n, labels = lg.weighted_clique_ring(cliques, size)
    comm, nc, q, rounds = _device(ctx, e, w, n)
    print(cliques, size, "device", nc, q, rounds, "formula", modularity(e, w, n, comm))
    assert nc == cliques + 2 and np.array_equal(comm, labels)
    assert q == pytest.approx(modularity(e, w, n, comm), abs=1e-12)
    comm2, _, q2, _ = ctx.louvain()
    assert modularity(e, w, n, comm2) == pytest.approx(modularity(e, w, n, comm), abs=1e-12) and q2 == pytest.approx(q, abs=1e-12)


def test_reference_fixture_against_the_restatement(ctx):
    e = np.loadtxt(os.path.join(GOLDEN, "test115", "test.edgelist"), dtype=np.int64)[:, :2]
    comm, nc, q, rounds = _device(ctx, e, None, 115)
    _, _, r_q, r_rounds = sync_level1(e, None, 115)
    print("device", nc, q, rounds, "restatement", r_q, r_rounds)
    assert q >= r_q and rounds == r_rounds
