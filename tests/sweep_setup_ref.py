"""The set-up of an alpha sweep in plain numpy and the standard library: what the testing hook cge_sweep_setup_test must give.

D, its extrema over j >= i and the normalisation are tests/packed_gd_ref.py's (dist_matrix, extrema_upper, normalised): every
step is an IEEE operation that numpy and the device round alike.  Here: the layout (the community CSR with ascending members is
the order of a relabelled sweep), the stored logarithm log2(fl(1 - D)) from `decimal` at 60 digits with the index function of its
tile-blocked layout, the start vectors with TT, and the degree pass of a directed edge list."""
import decimal

import numpy as np

from packed_gd_ref import dist_matrix, extrema_upper, normalised  # noqa: F401  (one definition for both suites)

LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------
# the layout
def layout(comm, C, relabel):
    """comm: ids in 1..C.  The community -> members CSR with ascending members; its member list is the order of a relabelled
    sweep (the vertex at each position of the sweep's numbering) and old2new its inverse.  cm_mem / cm_pos are the tables the
    device gets: in the sweep's numbering (the identity, after a relabel) or the CSR and its inverse."""
    comm = np.asarray(comm, dtype=np.int64)
    N = comm.size
    order = np.argsort(comm, kind="stable").astype(np.int32)
    cm_off = np.concatenate([[0], np.cumsum(np.bincount(comm - 1, minlength=C))]).astype(np.int32)
    old2new = np.empty(N, np.int32)
    old2new[order] = np.arange(N, dtype=np.int32)
    ident = np.arange(N, dtype=np.int32)
    return {"order": order, "old2new": old2new, "cm_off": cm_off, "cm_mem": ident if relabel else order,
            "cm_pos": ident if relabel else old2new, "perm": order if relabel else ident}


def tiles_apply(comm, C):
    """The tile form's statement: N >= 256, C >= 2 and at most 64 community ids in every 64-vertex block of the sorted order."""
    s = np.sort(np.asarray(comm))
    N = s.size
    spans = [s[min(N, b + 64) - 1] - s[b] + 1 for b in range(0, N, 64)]
    return N >= 256 and C >= 2 and max(spans) <= 64


# ---------------------------------------------------------------------------------------------------------------
# the logarithm
def upper_tile_mask(N):
    """The elements of the upper 64 x 64 tiles: tile row <= tile column, the diagonal tiles whole."""
    t = np.arange(N) // 64
    return t[:, None] <= t[None, :]


def blocked_count(N):
    Nt = (N + 63) // 64
    return Nt * (Nt + 1) // 2 * 4096


def blocked_index(N):
    """idx[r, c] = where element (r, c) of an upper tile sits in the tile-blocked layout (-1 outside the upper tiles): tile
    t = (I, J), I <= J, counted row by row over the upper tiles; lane 8 rq + cq holds rows 64 I + 8 rq + a and columns
    64 J + 8 cq + b at (t * 64 + lane) * 64 + 8 a + b."""
    Nt = (N + 63) // 64
    r, c = np.arange(N, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    I, J = r // 64, c // 64
    t = I * Nt - I * (I - 1) // 2 + (J - I)
    lane = 8 * ((r % 64) // 8) + (c % 64) // 8
    idx = (t * 64 + lane) * 64 + 8 * (r % 8) + c % 8
    return np.where(I <= J, idx, -1)


def log2_exact(x):
    """log2 of the doubles x (> 0, finite) as `decimal` numbers of 60 digits."""
    ctx = decimal.Context(prec=60)
    ln2 = ctx.ln(decimal.Decimal(2))
    return [ctx.divide(ctx.ln(decimal.Decimal(float(v))), ln2) for v in x]


def log2_rel_error(x, Lh, Ll):
    """|Lh + Ll - log2(x)| / |log2(x)| per element, as floats (0 where both are 0: x == 1)."""
    ctx = decimal.Context(prec=60)
    out = np.zeros(len(x))
    for k, (ref, h, l) in enumerate(zip(log2_exact(x), Lh, Ll)):
        err = abs(ctx.subtract(ctx.add(decimal.Decimal(float(h)), decimal.Decimal(float(l))), ref))
        out[k] = 0.0 if err == 0 else float(ctx.divide(err, abs(ref))) if ref != 0 else np.inf
    return out


# ---------------------------------------------------------------------------------------------------------------
# the start vectors
def start(N, deg_in=None, deg_out=None):
    """T1, T2 and TT (3, Tld): ones (undirected), or zero where the in- / out-degree is (directed: Tin, Tout); part 0 of TT holds
    T1, everything else of it is zero; Tld = 64 ceil(N / 64)."""
    T1 = np.ones(N) if deg_in is None else np.where(np.asarray(deg_in) == 0, 0.0, 1.0)
    T2 = np.ones(N) if deg_out is None else np.where(np.asarray(deg_out) == 0, 0.0, 1.0)
    Tld = (N + 63) // 64 * 64
    TT = np.zeros((3, Tld))
    TT[0, :N] = T1
    return T1, T2, TT, Tld


# ---------------------------------------------------------------------------------------------------------------
# the degrees of a directed edge list
def degrees(N, src, dst, w=None):
    """(deg_out, deg_in) as long doubles, star = the rows of the edge list each vertex appears in (a self-loop twice), and
    sum|w| per vertex and direction with the number of terms, for the bound of a sum in any order."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    w = np.ones(src.size, LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)
    out, inn = np.zeros(N, LD), np.zeros(N, LD)
    np.add.at(out, src, w)
    np.add.at(inn, dst, w)
    star = (np.bincount(src, minlength=N) + np.bincount(dst, minlength=N)).astype(np.int32)
    return out, inn, star, np.bincount(src, minlength=N), np.bincount(dst, minlength=N)


def degrees_sequential(N, src, dst, w=None):
    """The same sums in float64, edge by edge: for unit and dyadic weights every partial sum is exact, so any order gives these
    bits."""
    out, inn = np.zeros(N), np.zeros(N)
    for e in range(len(src)):
        we = 1.0 if w is None else float(w[e])
        out[src[e]] += we
        inn[dst[e]] += we
    return out, inn
