"""Plain numpy references of the fused chain's epilogue (csrc/fit_flow_body.inc): the layout and its tile tables, vect_B's tile
partials and bins in np.longdouble, the local score's tallies in float64, the fit's launch geometry.  Pinned on the CPU by
tests/test_fused_chain_ref.py; tests/test_gpu_fused_chain.py holds the device to them."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
NP = 32  # CGE_FLOW_NP: pieces per 64-vertex block at most
BLOCKS = 64  # CGE_PARTIAL_BLOCKS


def layout(comm, C):
    """layout_tables' rule for ids `comm` in 1..C (any vertex order, ids without a member allowed): the sweep numbers the
    vertices by community, members ascending.  Returns a dict: order (the caller's 0-based vertex at each position), comm_new
    (0-based ids in the sweep's numbering), Nt, fc / ns (first id and number of ids, empty ones included, of every 64-vertex
    block), base (Nt * Nt: where a tile's partials start; tiles below the diagonal hold none), bt_total, and pieces = per block
    one piece per 8-column chunk start and per change of community inside a chunk (the tail beyond N is a run)."""
    comm = np.asarray(comm, dtype=np.int64) - 1
    N = comm.size
    assert comm.min() >= 0 and comm.max() < C
    order = np.argsort(comm, kind="stable").astype(np.int32)
    cn = comm[order]
    Nt = (N + 63) // 64
    fc = np.array([cn[64 * b] for b in range(Nt)], dtype=np.int32)
    ns = np.array([cn[min(N, 64 * b + 64) - 1] - cn[64 * b] + 1 for b in range(Nt)], dtype=np.int32)
    pieces = []
    for b in range(Nt):
        n = 0
        for q in range(64):
            v = 64 * b + q
            cv = cn[v] if v < N else -1
            cu = (cn[v - 1] if v - 1 < N else -1) if q > 0 else -2
            n += (q & 7) == 0 or cv != cu
        pieces.append(n)
    base = np.zeros(Nt * Nt, dtype=np.int32)
    tot = 0
    for I in range(Nt):
        for J in range(Nt):
            base[I * Nt + J] = tot
            if J >= I:
                tot += int(ns[I]) * int(ns[J])
    return {"order": order, "comm_new": cn, "N": N, "C": C, "Nt": Nt, "fc": fc, "ns": ns, "base": base, "bt_total": tot,
            "pieces": np.array(pieces)}


def _runs(ids):
    """Starts of the runs of equal values in `ids` and the value of each run."""
    st = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    return st, ids[st]


def partials(GD, T, lay):
    """vect_B's tile partials in long double, with the number of terms of each: the partial of tile (I, J), row community a and
    column community b sits at base[I Nt + J] + (a - fc[I]) ns[J] + (b - fc[J]) and is the sum of (T_i T_j) GD_ij over the rows
    i of block I in a and the columns j of block J in b, j >= i when I = J, in the sweep's numbering.  GD, T: the caller's
    numbering (GD symmetric)."""
    o, cn, N, Nt, fc, ns, base = (lay[k] for k in ("order", "comm_new", "N", "Nt", "fc", "ns", "base"))
    G = LD(np.asarray(GD)[np.ix_(o, o)])
    t = LD(np.asarray(T)[o])
    val = np.zeros(lay["bt_total"], LD)
    cnt = np.zeros(lay["bt_total"], np.int64)
    for I in range(Nt):
        r0, r1 = 64 * I, min(N, 64 * I + 64)
        rs, ra = _runs(cn[r0:r1])
        for J in range(I, Nt):
            c0, c1 = 64 * J, min(N, 64 * J + 64)
            cs, cb = _runs(cn[c0:c1])
            P = (t[r0:r1, None] * t[None, c0:c1]) * G[r0:r1, c0:c1]
            live = np.ones(P.shape, np.int64)
            if I == J:
                live = np.triu(live)
                P = np.where(live > 0, P, LD(0))
            Z = np.add.reduceat(np.add.reduceat(P, rs, axis=0), cs, axis=1)
            K = np.add.reduceat(np.add.reduceat(live, rs, axis=0), cs, axis=1)
            pos = base[I * Nt + J] + (ra[:, None] - fc[I]) * int(ns[J]) + (cb[None, :] - fc[J])
            val[pos] = Z
            cnt[pos] = K
    return val, cnt


def fold(values, lay):
    """The tile partials (or their term counts) added into vect_B's packed bins (row-major upper triangle of the id pairs)."""
    cn, N, C, Nt, fc, ns, base = (lay[k] for k in ("comm_new", "N", "C", "Nt", "fc", "ns", "base"))
    Z = np.zeros((C, C), values.dtype)
    for I in range(Nt):
        for J in range(I, Nt):
            nI, nJ = int(ns[I]), int(ns[J])
            blk = values[base[I * Nt + J]:base[I * Nt + J] + nI * nJ].reshape(nI, nJ)
            Z[fc[I]:fc[I] + nI, fc[J]:fc[J] + nJ] += blk
    return _packed(Z)


def _packed(Z):
    """(C, C) sums by ordered id pair -> the packed vector: bin (min, max)."""
    C = Z.shape[0]
    B = Z + Z.T
    B[np.diag_indices(C)] = np.diag(Z)
    return B[np.triu_indices(C)]


def vect_b(GD, T, comm, C):
    """vect_B from its definition in the caller's numbering, in long double, with the number of terms per bin: bin
    (min(c_i, c_j), max(c_i, c_j)) accumulates (T_i T_j) GD_ij over i <= j."""
    c0 = np.asarray(comm, dtype=np.int64) - 1
    N = c0.size
    t = LD(np.asarray(T))
    live = np.triu(np.ones((N, N), bool))
    flat = (c0[:, None] * C + c0[None, :])[live]
    P = ((t[:, None] * t[None, :]) * LD(np.asarray(GD)))[live]
    Z = np.zeros(C * C, LD)
    np.add.at(Z, flat, P)
    K = np.bincount(flat, minlength=C * C)
    return _packed(Z.reshape(C, C)), _packed(K.reshape(C, C))


def _tally_terms(T, aidx, afac, ppos, pneg):
    T = np.asarray(T, dtype=np.float64)
    a = [(T[aidx[u]] * afac[2 * u]) / afac[2 * u + 1] for u in range(4)]
    return (a[0] * a[1]) * ppos, (a[2] * a[3]) * pneg


def tallies(T, aidx, afac, aden, wts, ppos, pneg):
    """auc_landmark_kernel's arithmetic in float64 on prepared operands: ai = (T[i] f0) / f1 and so on, pos = (ai aj) ppos,
    neg = (au av) pneg, num += (pos > neg) w.  Sample q belongs to block (q // 256) % 64; den[vb] = aden[vb].  Returns
    part (64, 2) = {num, den} per block.  (The test's weights make every sum exact, so the order of the additions is free.)"""
    pos, neg = _tally_terms(T, aidx, afac, ppos, pneg)
    S = pos.size
    blk = (np.arange(S) // 256) % BLOCKS
    part = np.zeros((BLOCKS, 2))
    np.add.at(part[:, 0], blk, np.where(pos > neg, 1.0, 0.0) * np.asarray(wts, dtype=np.float64))
    part[:, 1] = aden
    return part


def min_tally_gap(T, aidx, afac, ppos, pneg):
    """The smallest relative gap |pos - neg| / max(pos, neg) over the samples."""
    pos, neg = _tally_terms(T, aidx, afac, ppos, pneg)
    return float(np.min(np.abs(pos - neg) / np.maximum(pos, neg)))


def geometry(N, cus):
    """flow_geometry (kernels_fitp.hip): dict(Nt, NT, G, NW, NSB) or None = declined.  NSB == 1: the fused geometry."""
    if N <= 0 or N > 64 * 64 or cus <= 0:
        return None
    Nt = (N + 63) // 64
    NT = Nt * (Nt + 1) // 2
    NW = 4 if NT <= 4 * cus else 8
    G = min(cus, max((NT + NW - 1) // NW, 4 * Nt))
    if NT > NW * G or 4 * Nt > 2 * G:
        return None
    return {"Nt": Nt, "NT": NT, "G": G, "NW": NW, "NSB": 1 if 4 * Nt <= G else 2}


# ---- the shapes of tests/test_gpu_fused_chain.py: community sizes in id order (0: an id without a member) -----------------

def _random_sizes(total, C, seed):
    """C sizes in 1..120 summing to `total`, at least two of them 1."""
    rng = np.random.default_rng(seed)
    while True:
        s = rng.integers(1, 121, C)
        s[:2] = 1
        s[-1] += total - s.sum()
        if 1 <= s[-1] <= 120:
            rng.shuffle(s)
            return [int(x) for x in s]


def sizes(name):
    if name == "256x2":  # the smallest, boundaries on tile edges
        return [128, 128]
    if name == "257x5":  # the last tile is one column wide, the tail is a run
        return [70, 50, 64, 72, 1]
    if name == "321x3":  # ragged last tile
        return [100, 200, 21]
    if name == "513x8":  # one vertex in a tile of its own
        return [64, 64, 128, 64, 64, 64, 64, 1]
    if name == "700x17":  # mixed sizes: 1, 2, 63, 64, 65; the 200 spans four blocks
        return [63, 1, 64, 2, 65, 200] + [30] * 10 + [5]
    if name == "640x10e":  # ids 4 and 5 (1-based) empty
        return [64, 100, 60, 0, 0, 96, 64, 128, 64, 64]
    if name == "pieces32":  # 32 pieces in block 0: the limit
        return [2] * 32 + [64] * 3
    if name == "pieces33":  # 33: the fused form declines
        return [2] * 31 + [1, 1] + [64] * 3
    if name == "1100x600":  # ~35 ids per block: the fused form declines
        return [2, 2, 2, 2, 2, 1] * 100
    if name == "1985x40":  # (on 256 CUs) workgroups without a quarter block
        return _random_sizes(1985, 40, 1985)
    if name == "2817x50":  # (on 256 CUs) the 8-wave instance
        return _random_sizes(2817, 50, 2817)
    raise KeyError(name)


def shuffled_comm(name, seed):
    """The shape's ids (1-based) in a vertex order shuffled by a fixed seed."""
    s = sizes(name)
    comm = np.repeat(np.arange(len(s)), s) + 1
    np.random.default_rng(seed).shuffle(comm)
    return comm, len(s)


def tally_inputs(N, S, seed):
    """Synthetic prepared operands of the tally: aidx uniform in 0..N-1, afac uniform in [0.5, 2], dpos / dneg uniform in
    [0, 0.95], wts in {0.25, 0.5, .., 2} (every sum exact in any order), aden arbitrary."""
    rng = np.random.default_rng(seed)
    return {"aidx": rng.integers(0, N, (4, S)).astype(np.int32), "afac": rng.uniform(0.5, 2.0, (8, S)),
            "aden": rng.uniform(1.0, 100.0, BLOCKS), "dpos": rng.uniform(0.0, 0.95, S), "dneg": rng.uniform(0.0, 0.95, S),
            "wts": rng.integers(1, 9, S) * 0.25}
