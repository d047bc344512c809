"""Ensemble Clustering for Graphs (`cge_ecg`, csrc/kernels_louvain.hip) on the CPU -- TEST INFRASTRUCTURE, numpy only.

K members, each the synchronous level-1 pass `louvain_ref.sync_level1` on the graph with every vertex v renamed rank_r[v]
(a splitmix64 ordering per member and seed), read back through rank_r; the 2-core on adjacency entries (repeated edges are
separate entries, self loops are none); every edge reweighted  w_min + (1 - w_min) * c / K  (c: members with both ends in one
community) when both ends are in the 2-core and w_min otherwise; the hierarchy `louvain_levels_ref.levels` on those weights.
Shares no code with the library.  With K and 1 / w_min powers of two every weight is dyadic, so every sum is exact in any order
and the device is comparable to the bit.

Departures from the published algorithm (Poulin & Theberge), as the library's: the members are synchronous passes diversified by
relabelling alone, they use the graph's own weights, and the 2-core counts adjacency entries, not distinct neighbours."""
import numpy as np

from louvain_levels_ref import levels
from louvain_ref import modularity, sync_level1

_M = (1 << 64) - 1


def mix(x):
    """splitmix64 of a Python int, modulo 2^64."""
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def _mix_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def ranks(seed, r, n):
    """rank_r (n,) int64: the position of v among the vertices ordered by (mix(base ^ v), v)."""
    base = mix((int(seed) & _M) ^ mix(int(r)))
    v = np.arange(n, dtype=np.uint64)
    key = _mix_np(np.uint64(base) ^ v)
    order = np.lexsort((v, key))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return rank


def member(edges0, w, n, rank):
    """(comm (n,) renumbered in ascending order of the rank-space labels, n_comm, q, rounds) of one member."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    comm, nc, q, rounds = sync_level1(rank[e], w, n)
    return comm[rank], nc, q, rounds


def two_core(edges0, n):
    """(core (n,) bool, rounds): every vertex with fewer than 2 live adjacency entries goes, all of a round together; rounds
    counts the rounds that removed something."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    alive = np.ones(n, dtype=bool)
    rounds = 0
    while True:
        live = alive[e[:, 0]] & alive[e[:, 1]]
        deg = np.bincount(e[live].ravel(), minlength=n)
        rm = alive & (deg < 2)
        if not rm.any():
            return alive, rounds
        alive[rm] = False
        rounds += 1


def edge_weights(edges0, members, core, w_min):
    """(m,) the ECG weight of every edge, self loops included; `members` is (K, n)."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    members = np.asarray(members)
    K = members.shape[0]
    c = (members[:, e[:, 0]] == members[:, e[:, 1]]).sum(axis=0).astype(np.float64)
    both = core[e[:, 0]] & core[e[:, 1]]
    return np.where(both, w_min + (1.0 - w_min) * c / float(K), w_min)


def ecg(edges0, w, n, members=16, w_min=0.05, seed=0, final_level=-1, rank_of=None):
    """dict: comm (n,), n_comm, q (the ORIGINAL graph), q_ecg (the reweighted graph), weights (m,), members (K, n), member_nc,
    member_q, member_rounds, core (n,) bool, peel_rounds, levels.  `rank_of(r)` replaces the ranks (tests)."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    parts = [member(e, w, n, ranks(seed, r, n) if rank_of is None else rank_of(r)) for r in range(members)]
    mem = np.stack([p[0] for p in parts])
    core, peel_rounds = two_core(e, n)
    ew = edge_weights(e, mem, core, w_min)
    lv = levels(e, ew, n, max_levels=max(final_level, 0))
    comm, nc, q_ecg, _ = lv[-1]
    return dict(comm=comm, n_comm=nc, q=modularity(e, w, n, comm), q_ecg=q_ecg, weights=ew, members=mem,
                member_nc=[p[1] for p in parts], member_q=[p[2] for p in parts], member_rounds=[p[3] for p in parts], core=core,
                peel_rounds=peel_rounds, levels=len(lv))


def ari(a, b):
    """Adjusted Rand index of two labelings."""
    a, b = np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1]
    t = np.zeros((a.max() + 1, b.max() + 1))
    np.add.at(t, (a, b), 1.0)
    c2 = lambda x: x * (x - 1.0) / 2.0
    s, sa, sb, tot = c2(t).sum(), c2(t.sum(1)).sum(), c2(t.sum(0)).sum(), c2(float(len(a)))
    exp = sa * sb / tot
    return float((s - exp) / (0.5 * (sa + sb) - exp))
