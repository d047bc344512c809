"""The synchronous level-1 Louvain of csrc/kernels_louvain.hip (`k_louvain_level1`) round for round on the CPU, and the
modularity of a partition by the direct formula -- TEST INFRASTRUCTURE, numpy only, no device.

`sync_level1` shares no code with the library but uses the same expressions in the same order in fp64: on integer and
dyadic weights every sum is exact whatever its order (the library is built with -ffp-contract=off), so the gains, the
ties between them, the moves, the round count and the modularity are those of the device to the bit.  On general real
weights the sums may round differently and break a tie the other way; there only the quality is comparable.

Conventions (those of the library and of the oracle's `louvain_level1`): the adjacency holds every edge both ways,
repeated edges are separate entries, a self loop is kept aside in self[v] and counts once in k_v and once in "in"."""
import numpy as np


def _graph(edges0, w, n):
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if w is None else np.asarray(w, dtype=np.float64)
    loop = e[:, 0] == e[:, 1]
    self_w = np.zeros(n)
    np.add.at(self_w, e[loop, 0], w[loop])
    u, v, ww = e[~loop, 0], e[~loop, 1], w[~loop]
    row, col, aw = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([ww, ww])
    k = np.zeros(n)
    np.add.at(k, row, aw)  # the row sum ...
    k = k + self_w  # ... plus the self loop, once
    return row, col, aw, self_w, k


def _renumber(comm):
    ids, inv = np.unique(comm, return_inverse=True)  # ascending old id
    return inv.astype(np.int64), len(ids)


def sync_level1(edges0, w, n):
    """(comm renumbered 0.. (n,), n_comm, q, rounds) of `k_louvain_level1` for the 0-based edge list `edges0` (m, 2)
    with weights `w` (None: unit) on n vertices."""
    row, col, aw, self_w, k = _graph(edges0, w, n)
    m2 = k.sum()
    comm = np.arange(n, dtype=np.int64)
    vid = np.arange(n, dtype=np.uint64)
    turn_bit = (((vid * np.uint64(2654435761)) % np.uint64(1 << 32)) >> np.uint64(15)) & np.uint64(1)
    if not (m2 > 0.0 and len(row) > 0):
        # nothing to move: the singletons, with their own modularity when there is any weight (self loops only)
        q = float(self_w.sum() / m2 - (k * k).sum() / (m2 * m2)) if m2 > 0.0 else 0.0
        return comm, n, q, 0
    best_q, best_comm, since_best, rounds = -1e300, comm.copy(), 0, 0
    for rnd in range(200):
        rounds = rnd + 1
        tot = np.bincount(comm, weights=k, minlength=n)
        size = np.bincount(comm, minlength=n)
        # the weight from every vertex to every neighbouring community, as the partition stands at the start of the round
        pairs, inv = np.unique(row * n + comm[col], return_inverse=True)
        ws = np.bincount(inv, weights=aw, minlength=len(pairs))
        pv, pc = pairs // n, pairs % n
        is_own = pc == comm[pv]
        w_own = np.zeros(n)
        w_own[pv[is_own]] = ws[is_own]
        in_sum = (w_own + self_w).sum()
        own_inc = w_own - (tot[comm] - k) * k / m2
        # the other communities in ascending id, strict improvement only: the largest gain, the smallest id among equals
        ov, oc = pv[~is_own], pc[~is_own]
        inc = ws[~is_own] - tot[oc] * k[ov] / m2
        order = np.lexsort((oc, -inc, ov))
        ov, oc, inc = ov[order], oc[order], inc[order]
        first = np.ones(len(ov), dtype=bool)
        first[1:] = ov[1:] != ov[:-1]
        ov, oc, inc = ov[first], oc[first], inc[first]
        take = inc > own_inc[ov]
        best = comm.copy()
        best[ov[take]] = oc[take]
        # two singletons only merge towards the smaller id
        drop = (best != comm) & (size[comm] == 1) & (size[best] == 1) & (best > comm)
        best[drop] = comm[drop]
        wants = best != comm
        moves = wants & (turn_bit == np.uint64(rnd & 1))  # a vertex moves in every other round only
        q = float(in_sum / m2 - (tot[size > 0] * tot[size > 0]).sum() / (m2 * m2))  # of the partition the round started from
        if q > best_q + 1e-6:
            best_q, best_comm, since_best = q, comm.copy(), 0
        else:
            since_best += 1
            if since_best >= 3:
                break
        if not wants.any():  # (a vertex that only the turn rule holds back keeps the pass going)
            break
        comm = np.where(moves, best, comm)
    out, nc = _renumber(best_comm)
    return out, nc, best_q, rounds


def modularity(edges0, w, n, comm):
    """sum_c in_c / m2 - (tot_c / m2)^2 of the partition `comm` (n,), straight from the edge list in fp64."""
    e = np.asarray(edges0, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e)) if w is None else np.asarray(w, dtype=np.float64)
    comm = np.asarray(comm)
    loop = e[:, 0] == e[:, 1]
    k = np.zeros(n)
    np.add.at(k, e[:, 0], w)
    np.add.at(k, e[~loop, 1], w[~loop])
    m2 = k.sum()
    if not m2 > 0.0:
        return 0.0
    inside = comm[e[:, 0]] == comm[e[:, 1]]
    in_sum = 2.0 * w[inside & ~loop].sum() + w[loop].sum()
    _, lab = np.unique(comm, return_inverse=True)
    tot = np.bincount(lab, weights=k)
    return float(in_sum / m2 - (tot * tot).sum() / (m2 * m2))
