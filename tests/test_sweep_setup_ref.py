"""tests/sweep_setup_ref.py held to what can be said without a device: the index function of the tile-blocked logarithm against
a brute-force enumeration, the layout against its defining properties, the logarithm against exactly known values, and the star
counts of the degree pass against the one place the oracle shows them (wGCL_directed's star-graph return)."""
import numpy as np
import pytest

import sweep_setup_ref as ref


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nt", [1, 2, 5])
@pytest.mark.parametrize("ragged", [0, 1, 37])
def test_blocked_index_is_the_enumeration(Nt, ragged):
    """Tiles row by row over I <= J, 64 lanes per tile, 8 x 8 elements per lane row by row: the k-th element enumerated sits at k."""
    N = 64 * Nt - ragged
    idx = ref.blocked_index(N)
    k, seen = 0, 0
    for I in range(Nt):
        for J in range(I, Nt):
            for rq in range(8):
                for cq in range(8):
                    for a in range(8):
                        for b in range(8):
                            r, c = 64 * I + 8 * rq + a, 64 * J + 8 * cq + b
                            if r < N and c < N:
                                assert idx[r, c] == k, (r, c)
                                seen += 1
                            k += 1
    assert k == ref.blocked_count(N) == Nt * (Nt + 1) // 2 * 4096
    mask = ref.upper_tile_mask(N)
    assert seen == mask.sum() and (idx[~mask] == -1).all() and (idx[mask] >= 0).all()
    assert np.unique(idx[mask]).size == seen  # no two elements share a slot


def test_upper_tile_mask():
    m = ref.upper_tile_mask(130)
    assert m[0, 0] and m[63, 0] and m[0, 129] and m[64, 127] and m[127, 64] and m[129, 128]
    assert not m[64, 63] and not m[128, 0] and not m[129, 127]


# ---------------------------------------------------------------------------------------------------------------
def _comm(rng, N, C, empty=None, single=None):
    ids = [q for q in range(1, C + 1) if q != empty]
    comm = rng.choice([q for q in ids if q != single], N)
    comm[: len(ids)] = ids  # every id but `empty` has a member
    if single is not None:
        comm[comm == single] = ids[0] if ids[0] != single else ids[1]
        comm[0] = single
    return rng.permutation(comm)


@pytest.mark.parametrize("N, C", [(1, 1), (65, 3), (257, 5), (321, 37)])
@pytest.mark.parametrize("relabel", [False, True])
def test_layout_properties(N, C, relabel):
    rng = np.random.default_rng(N + C)
    comm = _comm(rng, N, C, empty=2 if C > 2 else None, single=C if C > 2 else None)
    lay = ref.layout(comm, C, relabel)
    order, old2new, off = lay["order"], lay["old2new"], lay["cm_off"]
    assert sorted(order) == list(range(N))  # a permutation
    assert (old2new[order] == np.arange(N)).all() and (order[old2new] == np.arange(N)).all()  # and its inverse
    assert off[0] == 0 and off[-1] == N and off.size == C + 1
    for q in range(C):
        mem = order[off[q]:off[q + 1]]
        assert (comm[mem] == q + 1).all() and (np.diff(mem) > 0).all()  # the community's members, ascending
        assert mem.size == (comm == q + 1).sum()
    if C > 2:
        assert off[2] == off[1] and off[C] - off[C - 1] == 1  # the id without a member, the community of one
    # the device's tables speak the sweep's numbering
    comm_sweep = comm[lay["perm"]]
    for q in range(C):
        assert (comm_sweep[lay["cm_mem"][off[q]:off[q + 1]]] == q + 1).all()
    assert (lay["cm_mem"][lay["cm_pos"]] == np.arange(N)).all()
    if relabel:
        assert (np.diff(comm_sweep) >= 0).all()  # every community a range of consecutive vertices


def test_tiles_apply():
    assert ref.tiles_apply(np.repeat(np.arange(1, 6), 60), 5)
    assert not ref.tiles_apply(np.repeat(np.arange(1, 6), 51), 5)  # 255 vertices
    assert not ref.tiles_apply(np.ones(300, int), 1)
    assert not ref.tiles_apply(np.concatenate([np.arange(1, 64), np.full(300, 65)]), 65)  # block 0 spans ids 1..65, one empty
    assert ref.tiles_apply(np.concatenate([np.arange(1, 64), np.full(300, 64)]), 64)  # 64 ids


# ---------------------------------------------------------------------------------------------------------------
def test_log2_reference_on_known_values():
    x = np.array([2.0 ** -60, 0.5, 1.0, 8.0, 2.0 ** -1022])
    exact = [float(v) for v in ref.log2_exact(x)]
    assert exact == [-60.0, -1.0, 0.0, 3.0, -1022.0]
    # a double-double that is log2(3) to 2^-105 passes 2^-100; its head alone misses by its rounding error
    h = float(np.log2(3.0))
    import decimal
    l = float(ref.log2_exact([3.0])[0] - decimal.Decimal(h))
    assert ref.log2_rel_error([3.0], [h], [l])[0] < 2.0 ** -100
    assert 2.0 ** -56 < ref.log2_rel_error([3.0], [h], [0.0])[0] < 2.0 ** -52
    assert ref.log2_rel_error([1.0], [0.0], [0.0])[0] == 0.0


def test_start_vectors():
    T1, T2, TT, Tld = ref.start(65)
    assert Tld == 128 and (T1 == 1).all() and (T2 == 1).all() and TT.shape == (3, 128)
    assert (TT[0, :65] == 1).all() and (TT[0, 65:] == 0).all() and (TT[1:] == 0).all()
    T1, T2, TT, Tld = ref.start(3, deg_in=[0.0, 2.0, 0.5], deg_out=[1.0, 0.0, 0.0])
    assert T1.tolist() == [0, 1, 1] and T2.tolist() == [1, 0, 0] and TT[0, :3].tolist() == [0, 1, 1] and Tld == 64


# ---------------------------------------------------------------------------------------------------------------
def _is_star(star, N):
    """wGCL_directed's star-graph rule on the star counts (src/divergence.jl:321-334)."""
    star = np.asarray(star)
    return bool(((star == N - 1).any() and star.sum() == 2 * (N - 1)) or ((star == 2 * (N - 1)).any() and (star == 2).sum() == N - 1))


def _oracle_len(N, src, dst):
    from oracle import oracle as orc

    rng = np.random.default_rng(0)
    m = len(src)
    edges = np.stack([np.asarray(src) + 1, np.asarray(dst) + 1], 1).astype(np.int64)
    have = set(zip(src, dst))
    neg = [(i, j) for i in range(N) for j in range(N) if i != j and (i, j) not in have][:8]
    S = len(neg)
    smp = (rng.integers(1, m + 1, S), np.array([p[0] + 1 for p in neg]), np.array([p[1] + 1 for p in neg]))
    out = orc.wGCL_directed(edges, np.ones(m), np.arange(N) % 2 + 1, rng.standard_normal((N, 3)), np.zeros(N), np.ones(N), [], [],
                            np.zeros((0, 2), np.int64), [], np.zeros((0, 0)), False, smp)
    return len(out)


@pytest.mark.parametrize("name", ["out-star", "in-star", "two-way star", "path", "star + chord"])
def test_star_counts_are_what_the_oracle_acts_on(name):
    N = 6
    hub, leaves = np.zeros(N - 1, int), np.arange(1, N)
    src, dst = {"out-star": (hub, leaves), "in-star": (leaves, hub),
                "two-way star": (np.concatenate([hub, leaves]), np.concatenate([leaves, hub])),
                "path": (np.arange(N - 1), np.arange(1, N)),
                "star + chord": (np.concatenate([hub, [1]]), np.concatenate([leaves, [2]]))}[name]
    star = ref.degrees(N, src, dst)[2]
    assert star.sum() == 2 * len(src)
    assert _is_star(star, N) == (name in ("out-star", "in-star", "two-way star"))
    assert _oracle_len(N, list(src), list(dst)) == (6 if _is_star(star, N) else 7)


def test_degrees_reference():
    src, dst, w = [0, 0, 2, 2, 2], [1, 0, 0, 0, 2], [0.25, 0.5, 1.0, 1.0, 0.75]
    out, inn, star, k_out, k_in = ref.degrees(4, src, dst, w)
    assert out.tolist() == [0.75, 0, 2.75, 0] and inn.tolist() == [2.5, 0.25, 0.75, 0]
    assert star.tolist() == [5, 1, 4, 0] and k_out.tolist() == [2, 0, 3, 0] and k_in.tolist() == [3, 1, 1, 0]
    so, si = ref.degrees_sequential(4, src, dst, w)
    assert (so == out).all() and (si == inn).all()
    uo, ui = ref.degrees_sequential(4, src, dst)
    assert uo.tolist() == [2, 0, 3, 0] and ui.tolist() == [3, 1, 1, 0]
