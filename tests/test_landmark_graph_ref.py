"""CPU tests of what the kernel-level tests of the landmark graph stage judge by (tests/landmark_graph_ref.py) and of the tiled
form's geometry (hook cge_wedge_geometry_test: host arithmetic only): the geometry of every N keeps its keys inside 16 bits, its
tiles over exactly N rows and BOTH passes' LDS inside what the launch is granted; plain fp64 numpy stays inside the reference's
bounds, seeded mistakes fall outside them; fed with the oracle's own assignment the reference reproduces the oracle's landmark
graph of tests/golden/test115."""
import ctypes as C

import numpy as np
import pytest

import landmark_graph_ref as lg
from cge.jl_amd import api

LDS_GRANT = 160 * 1024  # what the launch wrapper asks for both kernels (cge_allow_lds)


def _geometry_sweep(weighted, n_chunks):
    """every N in 1..65535 through the C hook; {N: (rshift, colbits, ntile, lds1, lds2)} of the accepted ones"""
    lib = api.load_library()
    ap, rs, cb = C.c_int(), C.c_int(), C.c_int()
    nt, l1, l2 = C.c_int64(), C.c_int64(), C.c_int64()
    fn, out = lib.cge_wedge_geometry_test, {}
    fn.argtypes = [C.c_int64, C.c_int, C.c_int64] + [C.c_void_p] * 6
    refs = [C.addressof(x) for x in (ap, rs, cb, nt, l1, l2)]
    for N in range(1, 65536):
        assert fn(N, weighted, n_chunks, *refs) == 0
        if ap.value:
            out[N] = (rs.value, cb.value, nt.value, l1.value, l2.value)
    fn.argtypes = None
    return out


@pytest.mark.parametrize("n_chunks", [1, 105, 1200])
@pytest.mark.parametrize("weighted", [0, 1])
def test_wedge_geometry_of_every_N(weighted, n_chunks):
    """For every accepted N: 16-bit keys, a column field that holds N, tiles that cover rows 0..N-1 and no more, both LDS sizes
    inside the grant, per-chunk tile offsets inside what pass 2 gathers.  Pass 1 keeps one counter per tile beside its 64 KB table
    slice: with one row per tile (unit weights beyond N = 8192) that is what limits N -- 4 (roundup(N, 1024) + 18) bytes fit up to
    N = 23552.  Before the geometry looked at pass 1, unit N = 23553..36320 were accepted with 163912..213064 bytes."""
    acc = _geometry_sweep(weighted, n_chunks)
    for N, (rs, cb, nt, l1, l2) in acc.items():
        assert rs >= 0 and cb >= 1 and rs + cb <= 16, (N, rs, cb)
        assert N <= 1 << cb, (N, cb)
        assert (nt - 1) << rs < N <= nt << rs, (N, rs, nt)
        assert 0 < l1 <= LDS_GRANT and 0 < l2 <= LDS_GRANT, (N, l1, l2)
        assert n_chunks * (nt + 1) <= 1 << 27, (N, nt)
        assert l2 == (4, 8)[weighted] * (N << rs) + 4 * (2 * 1024 + 32), (N, l2)
        assert l1 == 65536 + 4 * ((nt + 1023) // 1024 * 1024 + 18), (N, l1)
    # what is accepted: an unbroken range from 1 (the form never declines a small N); its end is the first N whose LDS or
    # offsets do not fit
    top = max(acc)
    assert sorted(acc) == list(range(1, top + 1))
    if n_chunks == 1:
        assert top == (18160 if weighted else 23552)  # weighted: 8 N + 8320 <= 150 KB (pass 2); unit: pass 1, as above
    assert acc[4000][:3] == ((1, 12, 2000) if weighted else (2, 12, 1000))  # the headline: 4 rows per tile with unit weights
    for N, R in ((8192, 2), (8193, 1)) if not weighted else ((4096, 2), (4097, 1)):  # the R = 2 -> 1 steps
        assert 1 << acc[N][0] == R


def test_wedge_geometry_declines_what_pass_two_cannot_gather():
    assert api.wedge_geometry_test(4000, 0, (1 << 27) // 1001) is not None
    assert api.wedge_geometry_test(4000, 0, (1 << 27) // 1001 + 1) is None
    assert api.wedge_geometry_test(0, 0, 10) is None and api.wedge_geometry_test(65536, 0, 10) is None
    assert api.wedge_geometry_test(100, 0, 0) is None
    lib = api.load_library()
    assert lib.cge_wedge_geometry_test(C.c_int64(5), 0, C.c_int64(1), None, None, None, None, None, None) == -7


# ---- the reference itself ---------------------------------------------------------------------------------------------------
def _small_graph(kind, seed=5):
    rng = np.random.default_rng(seed)
    n, m, N = 500, 6000, 23
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    src[:50] = dst[:50]  # self-loops
    src[50:100], dst[50:100] = dst[100:150], src[100:150]  # both orientations
    v2l0 = rng.integers(0, N, n)
    return src, dst, lg.edge_weights(kind, m, rng), v2l0, N


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("kind", ["unit", "dyadic", "general"])
def test_numpy_fp64_pair_sums_are_inside_the_bound(kind, directed):
    src, dst, w, v2l0, N = _small_graph(kind)
    flat = lg.pair_index(v2l0[src], v2l0[dst], N, directed)
    bins, S, k = lg.bin_sums(flat, w)
    got = np.bincount(flat, weights=w, minlength=N * N)  # plain fp64, sequential
    assert k.max() > 5 and k.sum() == len(w) and abs(S.sum() - w.astype(lg.LD).sum()) <= 1e-15 * w.sum()  # (no term lost)
    if kind == "general":
        r = lg.bins_ratio(got, bins, S, k)
        print(kind, directed, r)
        assert r <= 1.0
        back = np.zeros(N * N)
        np.add.at(back, flat[::-1], w[::-1])  # another order: other bits, the same bound
        assert not np.array_equal(back, got) and lg.bins_ratio(back, bins, S, k) <= 1.0
    else:
        assert np.array_equal(got, lg.dense(bins, S, N * N)) and lg.bins_ratio(got, bins, S, k) == 0.0
    W = got.reshape(N, N)
    if not directed:
        assert np.all(np.tril(W, -1) == 0)
    do, di, star = lg.degrees_ref(W)
    assert lg.degrees_ratio(W.sum(1), do) <= 1.0 and lg.degrees_ratio(W.sum(0), di) <= 1.0
    assert star.sum() == 2 * np.count_nonzero(W > 0) and lg.positive_ref(W, directed) == len(bins)
    # vect_C's layouts
    C_ = 9
    comm0 = v2l0 % C_
    pk = lg.pair_index(comm0[src], comm0[dst], C_, directed, packed=True)
    assert pk.max() < (C_ * C_ if directed else C_ * (C_ + 1) // 2)
    if not directed:
        from oracle import oracle as orc

        a, b = np.minimum(comm0[src], comm0[dst]), np.maximum(comm0[src], comm0[dst])
        assert all(pk[e] == orc.idx(C_, int(a[e]) + 1, int(b[e]) + 1) - 1 for e in range(0, len(pk), 97))


@pytest.mark.parametrize("mutation", ["dropped_edge", "min_max_swapped", "ignored_weights"])
@pytest.mark.parametrize("kind", ["dyadic", "general"])
def test_a_wrong_pair_matrix_falls_outside(kind, mutation):
    """What a wrong kernel would return: the last edge lost; the undirected pair filed under (max, min); every weight taken as 1"""
    src, dst, w, v2l0, N = _small_graph(kind)
    a, b = v2l0[src], v2l0[dst]
    bins, S, k = lg.bin_sums(lg.pair_index(a, b, N, False), w)
    if mutation == "dropped_edge":
        bad = np.bincount(lg.pair_index(a[:-1], b[:-1], N, False), weights=w[:-1], minlength=N * N)
    elif mutation == "min_max_swapped":
        bad = np.bincount(lg.pair_index(np.maximum(a, b), np.minimum(a, b), N, True), weights=w, minlength=N * N)
    else:
        bad = np.bincount(lg.pair_index(a, b, N, False), minlength=N * N).astype(np.float64)
    assert lg.bins_ratio(bad, bins, S, k) > 1.0
    assert not np.array_equal(bad, lg.dense(bins, S, N * N))


@pytest.mark.parametrize("cls", lg.CLASSES)
@pytest.mark.parametrize("d", [1, 17, 64])
def test_aggregate_reference_and_its_mutations(cls, d):
    X, w, comm0, v2l, N = lg.make_aggregate_problem(cls, d)
    mem = lg.members_of(v2l - 1, N)
    assert [len(r) for r in mem[:len(lg.AGG_SIZES)]] == list(lg.AGG_SIZES) and all(np.all(np.diff(r) > 0) for r in mem if len(r) > 1)
    assert sum((w[r] == 0).any() and w[r].sum() > 0 for r in mem) >= 5 and w[mem[-1]].sum() == 0
    lemb, lw, dii, lcomm = lg.aggregate_ref(X, w, comm0, mem)
    assert np.isnan(lemb[-1]).all() and np.isnan(dii[-1]) and lw[-1] == 0 and np.isfinite(lemb[:-1]).all() and np.isfinite(dii[:-1]).all()
    assert lg.same_bits(lemb, lemb.copy()) and not lg.same_bits(np.array([0.0]), np.array([-0.0]))
    assert lcomm[N - 2] == 9 and len(set(comm0[mem[N - 2]])) == 2
    # plain numpy (pairwise sums, another order of additions) is inside the reordered-sum bound, and so is the reference
    pos = list(range(N - 1))
    plain_c = np.stack([(w[r][:, None] * X[r]).sum(0) / w[r].sum() for r in mem[:-1]])
    plain_d = np.array([np.sqrt(((plain_c[l] - X[mem[l]]) ** 2).sum() / w[mem[l]].sum()) for l in pos])
    for c_, d_ in ((plain_c, plain_d), (lemb[:-1], dii[:-1])):
        rc, rd = lg.reorder_ratios(X, w, mem[:-1], c_, d_)
        print(cls, d, rc, rd)
        assert rc <= 1.0 and rd <= 1.0
    # a member list in another order: inside the bound, but other bits
    rev = [r[::-1] for r in mem]
    lemb2, lw2, dii2, lcomm2 = lg.aggregate_ref(X, w, comm0, rev)
    rc, rd = lg.reorder_ratios(X, w, mem[:-1], lemb2[:-1], dii2[:-1])
    assert rc <= 1.0 and rd <= 1.0
    big = [l for l in pos if len(mem[l]) >= 255]
    assert not lg.same_bits(dii[big], dii2[big]) and not lg.same_bits(lemb[big], lemb2[big])
    # lcomm from the first member: differs on the landmark that spans two communities
    assert lcomm2[N - 2] == 8 and not np.array_equal(lcomm, lcomm2)
    # a lost member, ignored weights: outside the bound
    lost = [r[:-1] if len(r) > 1 else r for r in mem[:-1]]
    lemb3, _, dii3, _ = lg.aggregate_ref(X, w, comm0, lost)
    assert max(lg.reorder_ratios(X, w, mem[:-1], lemb3, dii3)) > 1.0
    lemb4, _, dii4, _ = lg.aggregate_ref(X, np.ones_like(w), comm0, mem[:-1])
    assert max(lg.reorder_ratios(X, w, mem[:-1], lemb4, dii4)) > 1.0


def test_reference_reproduces_the_oracle_on_test115(test115):
    """v_to_l of the oracle's landmarks() in, its landmark graph out: edges, their weights and the landmarks' weights exactly
    (integers and sums of a few unit weights), centroids and d_ii inside the reordered-sum bound"""
    from oracle import oracle as orc

    t = test115
    dii, embed, cluster, ledges, lw_e, lweight, v2l = orc.landmarks(t["edges"], t["eweights"], t["vweights"], t["clusters"], t["comm"],
                                                                    t["embedding"], False, t["land"], t["forced"], t["method"], False)
    v2l = np.asarray(v2l).ravel().astype(np.int64)
    N = int(v2l.max())
    X, w = np.ascontiguousarray(t["embedding"], dtype=np.float64), np.asarray(t["vweights"], dtype=np.float64).ravel()
    comm0 = np.asarray(t["comm"])[:, 0].astype(np.int64) - 1
    mem = lg.members_of(v2l - 1, N)
    lemb, lw, dii_r, lcomm = lg.aggregate_ref(X, w, comm0, mem)
    assert np.array_equal(lw, lweight) and np.array_equal(lcomm + 1, np.asarray(cluster).ravel())
    rc, rd = lg.reorder_ratios(X, w, mem, np.asarray(embed).reshape(N, -1), dii)
    rc2, rd2 = lg.reorder_ratios(X, w, mem, lemb, dii_r)
    print("oracle", rc, rd, "reference", rc2, rd2, "same bits", lg.same_bits(lemb, np.asarray(embed).reshape(N, -1)), lg.same_bits(dii_r, dii))
    assert max(rc, rd, rc2, rd2) <= 1.0
    e = np.asarray(t["edges"]) - 1
    bins, S, k = lg.bin_sums(lg.pair_index(v2l[e[:, 0]] - 1, v2l[e[:, 1]] - 1, N, False), np.asarray(t["eweights"], dtype=np.float64).ravel())
    W = lg.dense(bins, S, N * N).reshape(N, N)
    a, b = np.nonzero(W > 0)  # row-major: the order of src/landmarks.jl:454-461
    assert np.array_equal(np.stack([a, b], 1) + 1, ledges) and np.array_equal(W[a, b], np.asarray(lw_e).ravel())
    assert lg.positive_ref(W, False) == len(ledges)


def test_the_graphs_of_the_gpu_tests_have_the_tiles_they_claim():
    n, s, d = lg.make_graph("small")
    assert (n, len(s)) == (3000, 20000) and lg.tile_census(s, d, n) == ({(0, 0): 20000}, 2)
    pairs = set(zip(s.tolist(), d.tolist()))
    assert (s == d).sum() >= 200 and len(pairs) < len(s) - 300 and sum((b, a) in pairs for a, b in pairs if a != b) >= 1600
    n, s, d = lg.make_graph("bounds")
    assert n == 140_000 and lg.tile_census(s, d, n) == ({(0, 1): 16384, (1, 2): 16385, (0, 4): 1}, 4)
    assert {0, 32767, 65536, 131071, 131072, n - 1} <= set(s.tolist()) and {32768, 65535, 65536, n - 1} <= set(d.tolist())
    in_a = (s < lg.UBLOCK) & (d // lg.VBLOCK == 1)
    assert not np.any((s[in_a] >= lg.VBLOCK) & (s[in_a] < 2 * lg.VBLOCK))  # the pair assignment files tile (0, 1) under one pair
    pair = dict(lg.assignments("bounds", n, 77, np.random.default_rng(0)))["pair"]
    assert np.all(pair[s[in_a]] == 1) and np.all(pair[d[in_a]] == 77)
    n, s, d = lg.make_graph("chunks")
    tiles, n_chunks = lg.tile_census(s, d, n)
    assert n == 2_200_000 and len(tiles) == n_chunks == 17 * 68 == 1156 and set(tiles.values()) == {4, 5} and len(s) == 5009
    for N in (2, 77, 4000):
        a = dict(lg.assignments("chunks", n, N, np.random.default_rng(0)))
        assert len(np.unique(a["sparse"])) < N and a["contiguous"].max() == N and np.all(np.diff(a["contiguous"]) >= 0)
