"""The Louvain hierarchy of csrc/kernels_louvain.hip (`k_louvain_levels`) on the CPU -- TEST INFRASTRUCTURE, numpy only.

`contract` restates the contraction of an edge list by a partition (`partition2graph_binary` of generic Louvain, in the
library's conventions): one edge per unordered pair of communities, its weight the sum over the fine edges between them,
and a self-loop edge (C, C) of weight 2 * (inner edges) + (self loops of its vertices).  `levels` then calls
`louvain_ref.sync_level1` on each contracted list under the level rule: the hierarchy ends at the first level whose
partition has as many communities as its graph has vertices (that level is not reported, except level 1) or at
max_levels > 0.

A self-loop edge counts once in k and once in "in", in the library and in `sync_level1` alike, so a level of the device
is, by construction, `sync_level1` of the contracted list: no second restatement of the rounds is needed.  On integer and
dyadic weights every sum is exact in any order, so every level is comparable to the bit."""
import numpy as np

import louvain_graphs as lg
from louvain_ref import sync_level1


def contract(edges0, w, n, comm, n_comm):
    """(edges (m', 2) int64 on the vertices 0 .. n_comm-1, weights (m',)) of the graph contracted by `comm` (n,).  Self-loop
    edges of weight zero (a community of one vertex without a loop) are left out."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if w is None else np.asarray(w, dtype=np.float64)
    comm = np.asarray(comm, dtype=np.int64)
    assert len(comm) == n
    cu, cv = comm[e[:, 0]], comm[e[:, 1]]
    loop = e[:, 0] == e[:, 1]
    inner = (cu == cv) & ~loop
    self_w = np.zeros(n_comm)
    np.add.at(self_w, cu[inner], 2.0 * w[inner])  # an inner edge is seen from both ends
    np.add.at(self_w, cu[loop], w[loop])  # an original self loop counts once
    outer = cu != cv
    lo, hi = np.minimum(cu[outer], cv[outer]), np.maximum(cu[outer], cv[outer])
    pairs, inv = np.unique(lo * n_comm + hi, return_inverse=True)
    pw = np.bincount(inv, weights=w[outer], minlength=len(pairs))
    loops = np.flatnonzero(self_w != 0.0)
    edges = np.concatenate([np.stack([pairs // n_comm, pairs % n_comm], axis=1), np.stack([loops, loops], axis=1)])
    return edges.astype(np.int64), np.concatenate([pw, self_w[loops]])


def levels(edges0, w, n, max_levels=0, graphs=None):
    """[(comm of the ORIGINAL vertices (n,), n_comm, q, rounds)] per reported level.  `graphs` (a list) receives
    (edges, weights, n, uncomposed comm) of every reported level's own graph."""
    out, comp = [], None
    e, ww, nn = np.asarray(edges0, dtype=np.int64).reshape(-1, 2), w, n
    while True:
        comm, nc, q, rounds = sync_level1(e, ww, nn)
        if out and nc == nn:  # nothing merged: not reported
            break
        comp = comm if comp is None else comm[comp]
        out.append((comp, nc, q, rounds))
        if graphs is not None:
            graphs.append((e, ww, nn, comm))
        if (max_levels > 0 and len(out) >= max_levels) or nc == nn:
            break
        e, ww = contract(e, ww, nn, comm, nc)
        nn = nc
    return out


def longest_segment(edges0, n):
    """The longest adjacency segment of the list as the library holds it: one entry per edge end, self loops aside."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    return int(np.bincount(e.ravel(), minlength=n).max()) if len(e) else 0


# ---- graphs -------------------------------------------------------------------------------------------------------------
def hub_and_pairs(P):
    """An 8-clique (the hub, vertices 0 .. 7) and 2P triangles; triangle t (vertices 8 + 3t + {0, 1, 2}) is tied by one edge
    from its vertex 0 to hub vertex t mod 8, and triangles 2i and 2i + 1 are tied by two edges: vertex 1 to vertex 1 and
    vertex 2 to vertex 2.  n = 8 + 6P, m = 28 + 10P.  Level 1 finds the triangles, level 2 pairs them, and the hub's
    coarse vertex keeps one long adjacency segment among short ones."""
    pairs = lg.clique(0, 8)
    for t in range(2 * P):
        b = 8 + 3 * t
        pairs += lg.clique(b, 3)
        pairs.append((b, t % 8))
    for i in range(P):
        a, b = 8 + 3 * (2 * i), 8 + 3 * (2 * i + 1)
        pairs += [(a + 1, b + 1), (a + 2, b + 2)]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2), 8 + 6 * P


def dyadic(edges0, seed):
    """Weights in {1/4, 2/4, .. 8/4}: `integers(1, 9) / 4` of default_rng(seed)."""
    return np.random.default_rng(seed).integers(1, 9, size=len(edges0)) / 4.0


def known_answers():
    """name -> (edges0, w, n, [communities per level]) -- the counts are pinned from this restatement."""
    rm, n_rm = lg.random_multigraph(300, seed=1)
    soc = lg.star_of_cliques(300)
    return {
        "ring30x5": (*_unit(lg.clique_chain(30, 5, ring=True)), [30, 16]),
        "ring64x4": (*_unit(lg.clique_chain(64, 4, ring=True)), [64, 30, 20]),
        "chain257x3": (*_unit(lg.clique_chain(257, 3)), [257, 122, 58, 31]),
        "random300": (rm, None, n_rm, [133, 53, 36, 31]),
        "random300_dyadic": (rm, dyadic(rm, 1), n_rm, [119, 51, 33]),
        "star_of_cliques300": (*_unit(soc), [300]),
        "star70": (*_unit(lg.star(70)), [1]),
        "path5": (*_unit(lg.path(5)), [2]),
    }


def _unit(g):
    return g[0], None, g[1]
