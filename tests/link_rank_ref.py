"""A plain reference of cge_link_rank (include/cge_hip.h) for tests/test_gpu_link_rank.py, on top of tests/link_ref.py: numpy and
long double, nothing of the kernels.

For a pair (i, j) with p* = p(i, j) and the admissible candidates A = {c : c != i, c != j, c not excluded by a resident edge}:
    greater = #{c in A : p(i, c) > p*},   ties = #{c in A : p(i, c) == p*},   cand = |A|.

  rank            brute force with link_ref.prob's long-double values, and the bracket the GPU test holds the device to:
                      lower = #{c in A : p_ref(c) > p*_ref (1 + 2 BOUND)},   upper = #{c in A : p_ref(c) >= p*_ref (1 - 2 BOUND)}.
                  A device value is within BOUND (relative) of the reference's, so p_ref(c) > p*_ref (1 + 2 BOUND) implies
                  p_dev(c) >= p_ref(c)(1 - BOUND) > p*_ref (1 + 2 BOUND)(1 - BOUND) ~ p*_ref (1 + BOUND) >= p*_dev (the second-order
                  term 2 BOUND^2 = 1e-30 is far below the long double's own 5e-20), i.e. lower <= greater_dev; likewise
                  p_dev(c) >= p*_dev implies p_ref(c) >= p*_ref (1 - 2 BOUND), i.e. greater_dev + ties_dev <= upper.  The bracket is
                  the issue's; nothing is chosen and no pair is left out.
  counts_of       the same three counts from ANY table of values (the device's own cge_link_prob values in the GPU test).
  scheme_counts   the device's bookkeeping restated: pairs grouped by query and sorted by p* descending; every admissible candidate
                  of the query (the pairs' own j among them) placed by binary search -- one increment of G at the first slot it
                  exceeds, one of E at the start of the run it equals; greater = the inclusive prefix sum of G, ties = E of the run
                  minus the pair's own j where that is admissible, cand from the excluded-neighbour counts.
"""
import numpy as np

import link_ref as lr

LD = np.longdouble


def _admissible_mask(i, n, nbrs, exclude):
    ok = np.ones(n, bool)
    ok[i] = False
    if exclude:
        ok[list(nbrs[i])] = False
    return ok


def counts_of(values, ok, j):
    """(greater, ties, cand) of target j from one query's table of values (n,) and its admissible mask (j itself is no candidate)."""
    ok = ok.copy()
    ok[j] = False
    v = values[ok]
    return int((v > values[j]).sum()), int((v == values[j]).sum()), int(ok.sum())


def rank(X, hi, alpha, f_out, f_in, i, j, edges=None, directed=False, exclude=True):
    """Brute force for the 0-based pairs: greater, ties, cand, lower, upper (int64 arrays; see the module's docstring)."""
    n = len(X)
    nbrs = lr.neighbours(edges if edges is not None else np.zeros((0, 2), np.int64), n, directed)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    out = np.zeros((5, len(i)), np.int64)
    tables = {}
    for q, (a, b) in enumerate(zip(i, j)):
        a, b = int(a), int(b)
        if a not in tables:
            tables[a] = (lr.prob(X, hi, alpha, f_out, f_in, np.full(n, a), np.arange(n)), _admissible_mask(a, n, nbrs, exclude))
        p, ok = tables[a]
        out[0, q], out[1, q], out[2, q] = counts_of(p, ok, b)
        ok = ok.copy()
        ok[b] = False
        out[3, q] = (p[ok] > p[b] * (1 + LD(2 * lr.BOUND))).sum()
        out[4, q] = (p[ok] >= p[b] * (1 - LD(2 * lr.BOUND))).sum()
    return tuple(out)


def excluded_counts(edges, n, directed):
    """Per vertex the distinct excluded neighbours other than itself, the way the device derives them: sorted keys, the first of
    every run of equal keys, self loops skipped, both ends of an undirected key and the source of a directed one."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    a, b = e[:, 0], e[:, 1]
    if not directed:
        a, b = np.minimum(a, b), np.maximum(a, b)
    keys = np.sort((a << 32) | b)
    first = np.ones(len(keys), bool)
    first[1:] = keys[1:] != keys[:-1]
    excl = np.zeros(n, np.int64)
    for k in keys[first]:
        u, v = int(k >> 32), int(k & 0xffffffff)
        if u == v:
            continue
        excl[u] += 1
        if not directed:
            excl[v] += 1
    return excl


def scheme_counts(values, n, i, j, edges=None, directed=False, exclude=True):
    """The device's scheme on `values(a)` -> the (n,) table of query a: returns (greater, ties, cand) in the caller's order."""
    edges = edges if edges is not None else np.zeros((0, 2), np.int64)
    nbrs = lr.neighbours(edges, n, directed)
    excl = excluded_counts(edges, n, directed) if exclude else np.zeros(n, np.int64)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    P = len(i)
    pstar = np.array([values(int(a))[int(b)] for a, b in zip(i, j)])
    perm = np.lexsort((np.arange(P), -pstar, i))  # by query, p* descending, the caller's order among equals
    t, gi, gj = pstar[perm], i[perm], j[perm]
    start = np.flatnonzero(np.r_[True, gi[1:] != gi[:-1]])
    off = np.r_[start, P]
    G, E = np.zeros(P, np.int64), np.zeros(P, np.int64)
    greater, ties, cand = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    for u in range(len(start)):
        a, o0, cnt = int(gi[off[u]]), off[u], off[u + 1] - off[u]
        tq = t[o0:o0 + cnt]
        ok = _admissible_mask(a, n, nbrs, exclude)
        for pc in values(a)[ok]:
            eq0 = int(np.searchsorted(-tq, -pc, side="left"))   # the first slot with t <= p_c
            s0 = int(np.searchsorted(-tq, -pc, side="right"))   # the first slot with t < p_c
            if s0 < cnt:
                G[o0 + s0] += 1
            if eq0 < s0:
                E[o0 + eq0] += 1
        pref = np.cumsum(G[o0:o0 + cnt])
        for s in range(cnt):
            run0 = int(np.searchsorted(-tq, -tq[s], side="left"))
            own = 1 if ok[gj[o0 + s]] else 0
            at = perm[o0 + s]
            greater[at] = pref[s]
            ties[at] = E[o0 + run0] - own
            cand[at] = n - 1 - excl[a] - own
    return greater, ties, cand


# ---- the inputs of tests/test_gpu_link_rank.py -------------------------------------------------------------------------------------
# (n, d, distinct queries, pairs per query, directed, exclude, seed): every n, d, Qu and pairs-per-query of the issue occurs, on
# both sides of the 128-row and 128-candidate tiles and of the finalisation's 64 slots a round; n = 2 is cand = 0; n = 1000 has
# eight candidate tiles, so several slices run.
RANK_SHAPES = [
    (2, 1, 1, 1, False, False, 1),
    (2, 16, 1, 63, False, True, 2),
    (127, 17, 127, 1, False, True, 3),
    (128, 40, 128, 64, True, True, 4),
    (129, 1, 129, 65, False, False, 5),
    (257, 16, 1, 300, True, False, 6),
    (257, 17, 128, 63, False, True, 7),
    (1000, 40, 1, 1, False, True, 8),
    (1000, 16, 300, 1, True, True, 9),
    (1000, 17, 129, 65, False, False, 10),
    (1000, 1, 127, 64, True, True, 11),
    (1000, 40, 300, 63, False, True, 12),
]


def shape_case(n, d, Qu, ppq, directed, exclude, seed):
    """link_ref.shape_case's input with Qu distinct queries and ppq pairs each (targets drawn with repeats), shuffled."""
    c = lr.shape_case(n, d, 1, 1, directed, exclude, seed)
    rng = np.random.default_rng(2000 + seed)
    qs = rng.permutation(n)[:Qu]
    i = np.repeat(qs, ppq)
    j = rng.integers(0, n - 1, len(i))
    j += j >= i  # any vertex but the query
    order = rng.permutation(len(i))
    c["i"], c["j"] = i[order].astype(np.int64), j[order].astype(np.int64)
    return c


def _with_pairs(c, i, j, **kw):
    c = dict(c)
    c.update(i=np.asarray(i, np.int64), j=np.asarray(j, np.int64), **kw)
    return c


def stress_cases():
    """link_ref.stress_cases' constructions with pairs to rank, and the cases of the issue that top-k has no use for."""
    s = lr.stress_cases()
    rng = np.random.default_rng(78)
    c = {}

    def targets(qs, n, per):
        i = np.repeat(np.asarray(qs, np.int64), per)
        j = rng.integers(0, n - 1, len(i))
        return i, j + (j >= i)

    # duplicated rows with equal factors: targets 5 and 105 tie exactly for every query; the same pair is given twice
    d = s["duplicated_rows"]
    qs = [q for q in d["queries"] if q not in (5, 105)]
    c["duplicated_rows"] = _with_pairs(d, np.r_[qs, qs, qs], np.r_[np.full(len(qs), 5), np.full(len(qs), 105), np.full(len(qs), 5)])
    e = s["equal_factors"]
    c["equal_factors"] = _with_pairs(e, *targets(e["queries"], 257, 3))
    f = s["far_heavy_vertex"]
    i, j = targets(f["queries"], 400, 2)
    c["far_heavy_vertex"] = _with_pairs(f, np.r_[i, f["queries"]], np.r_[j, np.full(len(f["queries"]), 399)])
    # a zero factor as query (3: every value is 0, everything survives and ties) and as target (50, 130)
    z = s["zero_factor"]
    c["zero_factor"] = _with_pairs(z, [3, 3, 4, 4, 199, 50, 4, 199], [7, 50, 50, 130, 3, 4, 199, 4])
    o = s["common_offset"]
    c["common_offset"] = _with_pairs(o, *targets(o["queries"], 600, 2))
    # the pair attaining the diameter: p* = 0, both ways, beside ordinary pairs of the same queries
    b = lr.shape_case(257, 17, 1, 1, False, True, 41)
    _, ai, aj = lr.diameter(b["X"])
    b["hi"] = lr.diameter(b["X"])[0]
    c["diameter_pair"] = _with_pairs(b, [ai, aj, ai, aj], [aj, ai, (ai + 1) % 257 if (ai + 1) % 257 != aj else (ai + 2) % 257,
                                                          (aj + 1) % 257 if (aj + 1) % 257 != ai else (aj + 2) % 257])
    # targets that are resident neighbours of their query under exclusion (undirected: either orientation; directed: both kinds)
    for directed in (False, True):
        g = lr.shape_case(300, 16, 1, 1, directed, True, 42 + directed)
        ed = g["edges"][g["edges"][:, 0] != g["edges"][:, 1]][:60]
        c[f"neighbour_targets_dir{int(directed)}"] = _with_pairs(g, np.r_[ed[:, 0], ed[:, 1]], np.r_[ed[:, 1], ed[:, 0]])
    # a hub query whose pairs are all n - 1 other vertices (a wave-wide scan with a carry), beside a few ordinary ones
    h = lr.shape_case(1000, 16, 1, 1, False, True, 44)
    others = np.delete(np.arange(1000), 17)
    i, j = targets([3, 500, 999], 1000, 2)
    c["hub"] = _with_pairs(h, np.r_[np.full(999, 17), i], np.r_[rng.permutation(others), j])
    # a supplied hi below the diameter: the base is clamped, many values are 0
    k = lr.shape_case(300, 8, 1, 1, False, True, 45)
    k["hi"] = 0.5 * lr.diameter(k["X"])[0]
    c["small_hi"] = _with_pairs(k, *targets(np.arange(0, 300, 7), 300, 3))
    return c
