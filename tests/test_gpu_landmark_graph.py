"""Kernel-level tests of the stage that turns an assignment v_to_l into the landmark graph (run with -m gpu on an MI355X), through
the hook cge_landmark_graph_test -- build_landmark_index + k_landmark_aggregate, the landmark-pair matrix by the tiled two-pass
form (k_wedge_scatter_blocked) and by k_edge_scatter + k_compact_count, the degrees of the directed score by k_wedge_degrees,
k_wedge_degrees_block and k_degrees_unpack -- and, for vect_C's blocked and tiled routes, through cge_edge_scatter, on
assignments the test chooses, against the references and a-priori bounds of tests/landmark_graph_ref.py (whose CPU tests show that
plain fp64 stays inside them and that a dropped edge, swapped min / max, ignored weights, another member order or lcomm of the
first member do not).

Three graphs (landmark_graph_ref.make_graph): `small` (one tile, two chunks), `bounds` (edges on the first and last vertex of
source and target blocks; tiles of exactly 16384, 16385 and 1 edges) and `chunks` (1156 tiles, so 1156 chunks: the second batch of
wedge_tile_kernel's chunk loop and gridDim.y = 5 in edge_row_reduce_kernel); unit, dyadic (k / 4) and general weights; directed
and undirected."""
import numpy as np
import pytest

import landmark_graph_ref as lg

pytestmark = pytest.mark.gpu

KINDS = ("unit", "dyadic", "general")
GRAPHS = ("small", "bounds", "chunks")
N_CHUNKS = {"small": 2, "bounds": 4, "chunks": 1156}
NS = (1, 2, 77, 255, 256, 257, 4000)
E_ARG = -7


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    c.resident = None
    yield c
    c.close()


@pytest.fixture(scope="module")
def graphs():
    """name -> dict(n, src, dst (0-based), edges (m, 2) 1-based, w[kind])"""
    out = {}
    for name in GRAPHS:
        n, src, dst = lg.make_graph(name)
        rng = np.random.default_rng([7, GRAPHS.index(name)])
        out[name] = {"name": name, "n": n, "src": src, "dst": dst, "edges": np.stack([src, dst], 1) + 1,
                     "w": {k: lg.edge_weights(k, len(src), rng) for k in KINDS}}
    return out


def _load(ctx, g, kind):
    """the graph with weights of `kind` resident on the context (kept across tests that ask for the same one)"""
    if ctx.resident != (g["name"], kind):
        ctx.set_graph(g["edges"], g["w"][kind], g["n"])
        ctx.resident = (g["name"], kind)
    return g["w"][kind]


def _share_chunks(n_chunks, part, nparts):
    return n_chunks * (part + 1) // nparts - n_chunks * part // nparts


def _geometry(out):
    return {k: out[k] for k in ("rshift", "colbits", "ntile")}


def _expected_geometry(N, kind, chunks):
    from cge.jl_amd import api

    geo = api.wedge_geometry_test(N, kind != "unit", max(chunks, 1))
    return None if geo is None else {k: geo[k] for k in ("rshift", "colbits", "ntile")}


def _check_matrix(W, bins, S, k, kind, directed, what):
    N = W.shape[0]
    if kind == "general":
        r = lg.bins_ratio(W, bins, S, k)
        assert r <= 1.0, (what, r)
    else:
        assert np.count_nonzero(W) == len(bins) and np.array_equal(W.ravel()[bins], S.astype(np.float64)), what
    if not directed and N <= 300:
        assert not np.any(np.tril(W, -1)) and not np.any(np.signbit(np.tril(W, -1))), what  # an exactly zero lower triangle
    # (beyond: every bin of the reference lies on or above the diagonal and nothing outside the bins is non-zero)
    assert directed or np.all(bins // N <= bins % N)


def _wedges_case(ctx, g, w, kind, directed, N, label, v2l, forms=(1, 2, 0)):
    what = (g["name"], kind, directed, N, label)
    bins, S, k = lg.bin_sums(lg.pair_index(v2l[g["src"]] - 1, v2l[g["dst"]] - 1, N, directed), w)
    geo = _expected_geometry(N, kind, N_CHUNKS[g["name"]])
    outs = {}
    for form in forms:
        out = outs[form] = ctx.landmark_graph_test(v2l, N, directed=directed, wedge_form=form)
        assert out["n_chunks"] == N_CHUNKS[g["name"]], what
        assert out["form_ran"] == (2 if form == 2 else 1), (what, form)
        assert _geometry(out) == (geo if form != 2 else {"rshift": -1, "colbits": -1, "ntile": -1}), (what, form)
        _check_matrix(out["wedges"], bins, S, k, kind, directed, (what, form))
        assert out["positive"] == len(bins), (what, form, out["positive"], len(bins))
    if kind != "general" and 2 in outs:  # the two forms bit for bit
        for form in forms:
            assert np.array_equal(outs[form]["wedges"], outs[2]["wedges"]), (what, form)
    return outs[forms[0]]


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gname", GRAPHS)
def test_wedges_tiled_form_against_the_reference_and_the_gather_form(ctx, graphs, gname, kind, directed):
    """The landmark-pair matrix by the tiled form (1), by gather + count (2) and by what a run picks (0: the tiled form) for N
    around a power of two, N = 1 (one tile of one row), R = 16384 ... 4 rows per tile, and every assignment of
    landmark_graph_ref.assignments: the matrix (exact for unit / dyadic weights, inside the reordered-sum bound otherwise), an
    exactly zero lower triangle, the positive count, the form that ran and the geometry the host-only hook gives."""
    g = graphs[gname]
    w = _load(ctx, g, kind)
    rng = np.random.default_rng([3, GRAPHS.index(gname), KINDS.index(kind), int(directed)])
    for N in NS:
        for label, v2l in lg.assignments(gname, g["n"], N, rng):
            if N == 4000 and label not in ("random", "contiguous"):
                continue
            _wedges_case(ctx, g, w, kind, directed, N, label, v2l, forms=(1, 2) if N == 4000 else (1, 2, 0))


@pytest.mark.parametrize("N,kind", [(8192, "unit"), (8193, "unit"), (4096, "general"), (4097, "general")])
def test_wedges_where_a_tile_goes_from_two_rows_to_one(ctx, graphs, N, kind):
    g = graphs["bounds"]
    w = _load(ctx, g, kind)
    v2l = np.random.default_rng(N).integers(1, N + 1, g["n"])
    out = _wedges_case(ctx, g, w, kind, False, N, "random", v2l, forms=(1,))
    assert 1 << out["rshift"] == (2 if N in (8192, 4096) else 1) and out["ntile"] == (N // 2 if N in (8192, 4096) else N)


def test_wedges_at_the_largest_N_of_the_tiled_form_and_one_beyond(ctx, graphs):
    """Unit weights, one row per tile: N = 23552 is the last N whose pass-1 counters fit the LDS grant (159816 of 163840 bytes);
    23553 goes to the gather form (the geometry declines; the tiled form named outright is CGE_E_ARG before any launch).  Only the
    positive count is read back (the matrices are 4.4 GB)."""
    from cge.jl_amd import api

    g = graphs["small"]
    _load(ctx, g, "unit")
    for N, form_ran in ((23552, 1), (23553, 2)):
        v2l = np.random.default_rng(N).integers(1, N + 1, g["n"])
        bins = np.unique(lg.pair_index(v2l[g["src"]] - 1, v2l[g["dst"]] - 1, N, True))
        out = ctx.landmark_graph_test(v2l, N, directed=True, wedge_form=0, wedges=False, positive=True)
        assert out["form_ran"] == form_ran and out["positive"] == len(bins), (N, out)
        assert _geometry(out) == ({"rshift": 0, "colbits": 15, "ntile": N} if form_ran == 1 else {"rshift": -1, "colbits": -1, "ntile": -1})
    with pytest.raises(api.CGEError) as e:
        ctx.landmark_graph_test(v2l, 23553, directed=True, wedge_form=1, wedges=False, positive=True)
    assert e.value.code == E_ARG and "tiled form declines" in str(e.value)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gname", ["small", "chunks"])
def test_wedges_of_the_parts_add_up(ctx, graphs, gname, kind):
    """The shares of 2, 3 and 7 pretend ranks (EdgeShare: of the chunks for the tiled form, of the edges for the gather form) add
    up to the whole; `small` has two chunks, so most of its seven tiled parts are empty and return zeros."""
    g = graphs[gname]
    w = _load(ctx, g, kind)
    N, nch = 77, N_CHUNKS[gname]
    v2l = np.random.default_rng(5).integers(1, N + 1, g["n"])
    for directed in (False, True):
        bins, S, k = lg.bin_sums(lg.pair_index(v2l[g["src"]] - 1, v2l[g["dst"]] - 1, N, directed), w)
        for form in (1, 2):
            for nparts in (2, 3, 7):
                total, empties = np.zeros((N, N), dtype=lg.LD), 0
                for part in range(nparts):
                    out = ctx.landmark_graph_test(v2l, N, directed=directed, wedge_form=form, part=part, nparts=nparts)
                    assert out["form_ran"] == form and out["positive"] == np.count_nonzero(out["wedges"] > 0)
                    if form == 1:
                        share = _share_chunks(nch, part, nparts)
                        assert _geometry(out) == _expected_geometry(N, kind, share)
                        if share == 0:
                            empties += 1
                            assert not out["wedges"].any() and out["positive"] == 0
                    total += out["wedges"]
                assert form == 2 or empties == (max(0, nparts - nch) if gname == "small" else 0)
                # (a bin's parts were each added in fp64 in some order and then here in long double: at most k - 1 roundings)
                if kind == "general":
                    assert lg.bins_ratio(total, bins, S, k) <= 1.0, (directed, form, nparts)
                else:
                    assert np.array_equal(total.ravel()[bins], S) and np.count_nonzero(total) == len(bins), (directed, form, nparts)


# ---- vect_C through cge_edge_scatter ------------------------------------------------------------------------------------------
def _vect_c_case(ctx, g, w, kind, directed, C_, comm):
    bins, S, k = lg.bin_sums(lg.pair_index(comm[g["src"]] - 1, comm[g["dst"]] - 1, C_, directed, packed=True), w)
    _, vc = ctx.edge_scatter(None, 1, C_, directed, want_wedges=False)
    if kind == "general":
        r = lg.bins_ratio(vc, bins, S, k)
        assert r <= 1.0, (g["name"], kind, directed, C_, r)
    else:
        assert np.array_equal(vc, lg.dense(bins, S, len(vc))), (g["name"], kind, directed, C_)
    return vc


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("kind", ["unit", "general"])
@pytest.mark.parametrize("gname", ["chunks", "bounds"])
def test_vect_c_blocked_and_tiled_routes(ctx, graphs, gname, kind, directed):
    """vect_C of the resident graph by the score path's forms: the row-bucketed two-pass form up to 2048 communities (on `chunks`
    its row reduction runs five batches of chunks), the tiled form of the landmark-pair matrix at 2049; community ids without a
    member among them."""
    g = graphs[gname]
    w = _load(ctx, g, kind)
    rng = np.random.default_rng([9, GRAPHS.index(gname)])
    for C_ in (1, 2, 37, 2048, 2049):
        comm = 2 * rng.integers(0, (C_ + 1) // 2, g["n"]) + 1 if C_ > 2 else rng.integers(1, C_ + 1, g["n"])  # (odd ids only)
        comm[-1] = C_
        ctx.set_vertex_data(comm, np.ones(g["n"]))
        _vect_c_case(ctx, g, w, kind, directed, C_, comm)


def test_the_two_forms_share_their_buffers_without_harm(ctx, graphs):
    """vect_C (blocked form), the landmark-pair matrix (tiled form), vect_C again on one context: the key and offset buffers are
    shared with other strides, and every result stays what it was (dyadic weights: exact sums, so the same bits); then a smaller
    graph of the other weight kind, whose results are its own."""
    g = graphs["chunks"]
    w = _load(ctx, g, "dyadic")
    rng = np.random.default_rng(21)
    comm = rng.integers(1, 38, g["n"])
    comm[-1] = 37
    ctx.set_vertex_data(comm, np.ones(g["n"]))
    v2l = rng.integers(1, 258, g["n"])
    vc1 = _vect_c_case(ctx, g, w, "dyadic", False, 37, comm)
    w1 = _wedges_case(ctx, g, w, "dyadic", False, 257, "random", v2l, forms=(1,))
    vc2 = _vect_c_case(ctx, g, w, "dyadic", False, 37, comm)
    w2 = _wedges_case(ctx, g, w, "dyadic", False, 257, "random", v2l, forms=(1,))
    vc3 = _vect_c_case(ctx, g, w, "dyadic", True, 37, comm)
    w3 = _wedges_case(ctx, g, w, "dyadic", False, 257, "random", v2l, forms=(1,))
    assert np.array_equal(vc1, vc2) and vc3.shape == (37 * 37,)
    assert all(np.array_equal(w1["wedges"], x["wedges"]) and w1["positive"] == x["positive"] for x in (w2, w3))
    s = graphs["small"]
    ws = _load(ctx, s, "unit")
    comm_s, v2l_s = rng.integers(1, 38, s["n"]), rng.integers(1, 258, s["n"])
    comm_s[-1] = 37
    ctx.set_vertex_data(comm_s, np.ones(s["n"]))
    _wedges_case(ctx, s, ws, "unit", False, 257, "random", v2l_s, forms=(1, 2))
    _vect_c_case(ctx, s, ws, "unit", False, 37, comm_s)
    _wedges_case(ctx, s, ws, "unit", True, 257, "random", v2l_s, forms=(1, 2))


def test_the_same_call_twice_gives_the_same_exact_sums(ctx, graphs):
    g = graphs["bounds"]
    w = _load(ctx, g, "dyadic")
    v2l = dict(lg.assignments("bounds", g["n"], 256, np.random.default_rng(0)))["pair"]
    a = ctx.landmark_graph_test(v2l, 256, wedge_form=1)
    comm = np.random.default_rng(1).integers(1, 38, g["n"])
    ctx.set_vertex_data(comm, np.ones(g["n"]))
    ctx.edge_scatter(None, 1, int(comm.max()), False, want_wedges=False)
    b = ctx.landmark_graph_test(v2l, 256, wedge_form=1)
    assert np.array_equal(a["wedges"], b["wedges"]) and a["positive"] == b["positive"] == 2
    assert a["wedges"][0, 255] == w[(g["src"] < lg.UBLOCK) & (g["dst"] // lg.VBLOCK == 1)].sum()  # 16384 additions into one cell


# ---- degrees ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 4000])
def test_degrees_of_the_landmark_pair_matrix(ctx, graphs, N, kind):
    """k_wedge_degrees on the returned matrix, and the block form for 1, 2, 3 and 7 pretend ranks (N = 2 over 3 ranks: an empty
    block): the blocks' star shares add up exactly, their sums are exact for unit / dyadic weights and inside the bound of a sum of
    N terms otherwise, and k_degrees_unpack of the blocks' sum is the whole."""
    g = graphs["small"]
    _load(ctx, g, kind)
    v2l = np.random.default_rng([4, N]).integers(1, N + 1, g["n"])
    exact = kind != "general"

    def judge(got, ref, terms, what):
        if exact:
            assert np.array_equal(got, ref.astype(np.float64)), what
        else:
            assert lg._ratio(got.astype(lg.LD) - ref, lg.sum_bound(ref, np.full(len(ref), terms))) <= 1.0, what

    first = None
    for world in (1, 2, 3, 7):
        # (every call makes its own matrix -- with general weights not the same bits twice -- and is judged on the one it returns)
        out = ctx.landmark_graph_test(v2l, N, directed=True, degrees=True, world=world)
        W = out["wedges"]
        do, di, star = lg.degrees_ref(W)
        assert np.array_equal(out["star"], star)
        judge(out["deg_out"], do, N, "deg_out")
        judge(out["deg_in"], di, N, "deg_in")
        blk = out["deg_block"].reshape(world, 3, N)
        per = (N + world - 1) // world
        for r in range(world):
            r0, r1 = min(N, per * r), min(N, per * (r + 1))
            rows = W[r0:r1]
            assert not blk[r, 0, :r0].any() and not blk[r, 0, r1:].any()
            sh = np.zeros(N)
            sh[r0:r1] = (rows > 0).sum(1)
            assert np.array_equal(blk[r, 2], sh + (rows > 0).sum(0)), (world, r)  # this block's share of the star counts
            judge(blk[r, 0, r0:r1], rows.astype(lg.LD).sum(1), N, (world, r, "rows"))
            judge(blk[r, 1], rows.astype(lg.LD).sum(0), max(r1 - r0, 1), (world, r, "columns"))
        if N == 2 and world == 3:
            assert not blk[2].any()
        assert np.array_equal(blk[:, 2].sum(0), star) and np.array_equal(out["u_star"], star)
        acc = np.zeros((3, N))
        for r in range(world):  # (the ranks' sum, in rank order)
            acc = acc + blk[r]
        assert np.array_equal(out["u_deg_out"], acc[0]) and np.array_equal(out["u_deg_in"], acc[1])
        judge(out["u_deg_out"], do, N, "u_deg_out")
        judge(out["u_deg_in"], di, N + world, "u_deg_in")  # (partial sums over N rows in all, then world - 1 more additions)
        if exact:
            assert np.array_equal(out["u_deg_out"], out["deg_out"]) and np.array_equal(out["u_deg_in"], out["deg_in"])
            first = first or out
            assert all(np.array_equal(out[k], first[k]) for k in ("wedges", "deg_out", "deg_in", "star"))


# ---- aggregate ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def actx():
    """a context without a graph: the aggregate needs the embedding and the vertex data only"""
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _aggregate(actx, X, w, comm0, v2l, N):
    actx.set_vertex_data(comm0 + 1, w)
    actx.set_embedding(X)
    return actx.landmark_graph_test(v2l, N, aggregate=True, wedges=False)


def _assert_aggregate(out, ref, what):
    lemb, lw, dii, lcomm = ref
    assert lg.same_bits(out["lweight"], lw), what
    assert lg.same_bits(out["lemb"], lemb), (what, np.argwhere(out["lemb"] != lemb)[:4])
    assert lg.same_bits(out["dii"], dii), (what, out["dii"], dii)
    assert np.array_equal(out["lcomm"], lcomm), what


@pytest.mark.parametrize("d", lg.AGG_WIDTHS)
@pytest.mark.parametrize("cls", lg.CLASSES)
def test_aggregate_bit_for_bit(actx, cls, d):
    """Centroids, weights, d_ii and communities against the sequential fp64 reference, bit for bit: landmarks of 1 ... 513
    members (the 8- and 16-row unrolls, the 256-member staging chunk +- 1, three chunks), widths around the four-columns-per-thread
    steps and beyond 1024 (the older kernel), zero weights inside a landmark, a landmark over two communities, one of zero weight
    (NaN for NaN).  A second call gives the same bits."""
    X, w, comm0, v2l, N = lg.make_aggregate_problem(cls, d)
    ref = lg.aggregate_ref(X, w, comm0, lg.members_of(v2l - 1, N))
    out = _aggregate(actx, X, w, comm0, v2l, N)
    _assert_aggregate(out, ref, (cls, d))
    assert np.isnan(out["dii"][-1]) and np.isnan(out["lemb"][-1]).all() and out["lweight"][-1] == 0
    again = actx.landmark_graph_test(v2l, N, aggregate=True, wedges=False)
    assert all(lg.same_bits(out[k], again[k]) for k in ("lemb", "lweight", "dii")) and np.array_equal(out["lcomm"], again["lcomm"])


@pytest.mark.parametrize("cls", lg.CLASSES)
def test_aggregate_kernels_of_both_widths_agree(actx, cls):
    """d = 1025 (landmark_aggregate_kernel) and the same data cut to d = 1024 (landmark_aggregate2_kernel): the centroid columns
    they share, the weights and the communities bit for bit"""
    X, w, comm0, v2l, N = lg.make_aggregate_problem(cls, 1025)
    wide = _aggregate(actx, X, w, comm0, v2l, N)
    cut = _aggregate(actx, np.ascontiguousarray(X[:, :1024]), w, comm0, v2l, N)
    assert lg.same_bits(wide["lemb"][:, :1024], cut["lemb"]) and lg.same_bits(wide["lweight"], cut["lweight"])
    assert np.array_equal(wide["lcomm"], cut["lcomm"])
    _assert_aggregate(cut, lg.aggregate_ref(np.ascontiguousarray(X[:, :1024]), w, comm0, lg.members_of(v2l - 1, N)), (cls, "cut"))


# ---- argument rules -----------------------------------------------------------------------------------------------------------
def test_argument_rules(ctx, actx, graphs):
    from cge.jl_amd import api

    g = graphs["small"]
    _load(ctx, g, "unit")
    v2l = np.random.default_rng(2).integers(1, 11, g["n"])

    def refused(c, text, *a, **kw):
        with pytest.raises(api.CGEError) as e:
            c.landmark_graph_test(*a, **kw)
        assert e.value.code == E_ARG and "landmark_graph_test" in str(e.value) and text in str(e.value), str(e.value)

    bad = v2l.copy()
    bad[17] = 11
    refused(ctx, "outside 1..10", bad, 10)
    bad[17] = 0
    refused(ctx, "outside 1..10", bad, 10)
    refused(ctx, "part 3 of 3", v2l, 10, part=3, nparts=3)
    refused(ctx, "embedding", v2l, 10, aggregate=True)  # (this context holds a graph only)
    X, w, comm0, v2l_a, N = lg.make_aggregate_problem("centred", 5)
    actx.set_vertex_data(comm0 + 1, w)
    actx.set_embedding(X)
    refused(actx, "graph is not resident", v2l_a, N)  # (and this one no graph)
    refused(actx, "has no member", v2l_a, N + 1, aggregate=True, wedges=False)
    out = ctx.landmark_graph_test(v2l, 12)  # landmarks 11 and 12 without a member: fine for the matrix
    assert out["form_ran"] == 1 and not out["wedges"][10:].any() and not out["wedges"][:, 10:].any()
