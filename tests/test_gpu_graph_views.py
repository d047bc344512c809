"""Graph views on the GPU (`pytest -m gpu`): cge_set_graph_view / cge_set_vertex_view take the edge list and the vertex data as the
caller holds them -- int32 / int64, 0- or 1-based, (2, m) / (m, 2) / sliced, host or device -- and derive the vertex weights and
the clusters.  Every comparison is bitwise: the resident tables (cge_resident_graph_test) are those `set_graph` /
`set_vertex_data` leave for the same edges as 1-based int64 columns, the derived vweight has the bits of the reference's loop
(src/auxilary.jl:104-110, `np.add.at` in args.py), and scores, traces and iteration counts are those of `set_inputs` + `score`."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, _parse

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1027, 16385, 70001)  # one edge, a partial wave, tails behind 16-byte loads, the edge passes' chunk + 1, many workgroups
N_IDS, N_VERT = 1000, 1003  # ids 1..1000 occur; 1001..1003 are trailing isolated vertices


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same_graph(got, ref):
    assert (got["n"], got["m"], got["unit"]) == (ref["n"], ref["m"], ref["unit"])
    assert np.array_equal(got["src"], ref["src"]) and np.array_equal(got["dst"], ref["dst"])
    assert (got["w"] is None) == (ref["w"] is None)
    if ref["w"] is not None:
        assert np.array_equal(_bits(got["w"]), _bits(ref["w"]))


def _same_trace(got, ref):
    """Every alpha's divergence and AUC (an entry that was not computed is a NaN on both sides) and the iteration counts."""
    assert got["n_alpha"] == ref["n_alpha"] and got["iters"] == ref["iters"]
    for key in ("div", "auc"):
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(_bits(g)[~np.isnan(r)], _bits(r)[~np.isnan(r)]), key


_cases = {}


def _case(ctx, m, wkind):
    """(1-based int64 (m, 2) edges, weights as the view gets them, the resident graph `set_graph` leaves), made once per shape."""
    key = (m, wkind)
    if key not in _cases:
        rng = np.random.default_rng(1000 + m)
        e = rng.integers(1, N_IDS + 1, size=(m, 2)).astype(np.int64)
        e[0] = (1, N_IDS)  # the extrema occur (what base = -1 and n = 0 infer from)
        w = {"none": None, "f64": 3 * rng.random(m) + 0.1, "f32": (3 * rng.random(m) + 0.1).astype(np.float32),
             "ones": np.ones(m)}[wkind]
        ctx.set_graph(e, np.ones(m) if w is None else w.astype(np.float64), N_VERT)
        _cases[key] = (e, w, ctx.resident_graph())
    return _cases[key]


def _held(e, w, dt, device, layout, base):
    """The edges as a caller might hold them: ids of `base`, dtype `dt`, (2, m) / (m, 2) / a slice [:, 1:] of a (2, m + 1) array,
    numpy on the host or a torch tensor on the GPU; the weights in the same place."""
    import torch

    ids = (e - 1 + base).astype(dt)
    if layout == "2xm":
        a = np.ascontiguousarray(ids.T)
    elif layout == "mx2":
        a = np.ascontiguousarray(ids)
    else:
        a = np.full((2, ids.shape[0] + 1), -7, dtype=dt)  # (column 0 holds an id that must never be read as one)
        a[:, 1:] = ids.T
    if device:
        a = torch.from_numpy(a).cuda()
        w = None if w is None else torch.from_numpy(w).cuda()
    return (a[:, 1:] if layout == "slice" else a), w


# ---- 1. ingest, element-exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["2xm", "mx2", "slice"])
@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=["int32", "int64"])
def test_view_leaves_the_resident_graph_of_set_graph(ctx, dt, device, layout):
    for m in SIZES:
        for wkind in ("none", "f32", "f64", "ones"):
            e, w, ref = _case(ctx, m, wkind)
            assert ref["unit"] == (wkind in ("none", "ones")) and ref["n"] == N_VERT and ref["m"] == m
            for base in (0, 1, -1):
                a, wv = _held(e, w, dt, device, layout, max(base, 0))
                assert ctx.set_graph_view(a, wv, n=N_VERT, base=base) == N_VERT
                got = ctx.resident_graph()
                try:
                    _same_graph(got, ref)
                except AssertionError as ex:
                    raise AssertionError(f"m={m} weights={wkind} base={base}: {ex}") from None


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_vertex_count_and_base_are_inferred(ctx, device):
    """n = 0: the maximum id (src/auxilary.jl:99); base = -1 on 1-based ids; both against `set_graph` with that n."""
    for m in SIZES:
        e, _, _ = _case(ctx, m, "none")
        ctx.set_graph(e, np.ones(m), N_IDS)
        ref = ctx.resident_graph()
        for base, dt, layout in ((-1, np.int32, "2xm"), (0, np.int64, "mx2"), (1, np.int64, "slice"), (-1, np.int64, "mx2")):
            for shift in ((0, 1) if base < 0 else (base,)):  # base = -1 decides 0 and 1 alike
                a, _ = _held(e, None, dt, device, layout, shift)
                assert ctx.set_graph_view(a, n=0, base=base) == N_IDS and ctx.n == N_IDS
                _same_graph(ctx.resident_graph(), ref)


# ---- 2. errors ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known115(ctx, test115):
    a = test115
    ctx.set_inputs(a["edges"], a["eweights"], a["vweights"], a["comm"], a["embedding"])
    return ctx.score(a["clusters"], a["land"], a["forced"], a["method"], seed=3, auc_samples=2000)


def _scores_correctly(ctx, a, known):
    ctx.set_inputs(a["edges"], a["eweights"], a["vweights"], a["comm"], a["embedding"])
    got = ctx.score(a["clusters"], a["land"], a["forced"], a["method"], seed=3, auc_samples=2000)
    assert np.array_equal(_bits(got), _bits(known))


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_bad_ids_are_refused_before_anything_is_indexed(ctx, test115, known115, device):
    import torch

    from cge.jl_amd import api

    m, n = 70001, 500
    rng = np.random.default_rng(5)
    good = rng.integers(1, n + 1, size=(2, m)).astype(np.int64)
    good[:, 0] = (1, n)

    def attempt(ids, base, n_arg, code, text, exc=api.CGEError):
        a = torch.from_numpy(ids).cuda() if device else ids
        with pytest.raises(exc) as ei:
            ctx.set_graph_view(a, n=n_arg, base=base)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
        assert ctx.resident_graph()["m"] == 0  # no graph is resident ...
        _scores_correctly(ctx, test115, known115)  # ... and the context goes on working

    bad = good.copy()
    for row in (1, m // 2, m):  # first, middle and last edge at once: the lowest row is named
        bad[row % 2, row - 1] = n + 1
    attempt(bad, 1, n, -7, "edge 1 has a vertex id outside 1..500")
    bad = good.copy()
    bad[0, m // 2 - 1] = n + 1
    bad[1, m - 1] = n + 7
    attempt(bad, 1, n, -7, f"edge {m // 2} has")
    bad = good.copy()
    bad[1, m - 1] = n + 1  # id = n + 1 at the last edge
    attempt(bad, 1, n, -7, f"edge {m} has")
    bad = good.copy() - 1
    bad[0, 4] = -1  # id = -1 (0-based)
    attempt(bad, 0, n, -7, "edge 5 has a vertex id outside 0..499")
    bad = good.copy()
    bad[1, 77] = 2**32 + 1  # on the 64-bit value: not vertex 1
    attempt(bad, 1, n, -7, "edge 78 has")
    attempt(bad, 1, 0, -7, "vertex count")  # ... nor a vertex count to infer
    attempt(good + 1, -1, n + 1, -1, "Vertices should be either 0-based or 1-based", api.AssertionErrorCGE)  # minimum id 2
    attempt(good.astype(np.int32) + 1, -1, 0, -1, "Vertices should be either 0-based or 1-based", api.AssertionErrorCGE)


def test_host_pointer_declared_on_device_is_refused(ctx, test115, known115):
    from cge.jl_amd import api

    ids = np.arange(1, 21, dtype=np.int64).reshape(2, 10)
    for with_w in (0, 1):
        g, keep, m = api.graph_view(ids, np.ones(10) * 2 if with_w else None, base=1)
        g.on_device = 1
        rc = ctx.L.cge_set_graph_view(ctx.h, C.byref(g), C.c_int64(m), C.c_int64(20), None)
        assert rc == -7 and "not device memory" in ctx.L.cge_last_error(ctx.h).decode()
    v, keep, n = api.vertex_view(np.ones(115, dtype=np.int64))
    v.on_device = 1
    assert ctx.L.cge_set_vertex_view(ctx.h, C.byref(v), C.c_int64(n)) == -7
    _scores_correctly(ctx, test115, known115)


# ---- 3. derived vertex weights --------------------------------------------------------------------------------------------------------
def _hub_graph():
    n, m = 300, 70001
    rng = np.random.default_rng(7)
    e = rng.integers(1, n, size=(m, 2)).astype(np.int64)  # ids 1..n-1: vertex n is isolated
    w = 3 * rng.random(m) + 0.1
    e[::3, 0] = 1  # a hub: every third edge leaves vertex 1
    e[::1000, 1] = e[::1000, 0]  # self-loops
    return n, m, e, w


def _reference_vw(n, e, w):
    vw = np.zeros(n)
    np.add.at(vw, e.ravel() - 1, np.repeat(w, 2))  # the order of args.py: u, v of edge 1, u, v of edge 2, ...
    return vw


@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
def test_derived_vertex_weights_have_the_bits_of_the_sequential_sum(ctx, device):
    import torch

    n, m, e, w = _hub_graph()
    ref = _reference_vw(n, e, w)
    # non-vacuity: the sum is order-sensitive on this input -- an unordered kernel could not pass by accident
    rev = _reference_vw(n, e[::-1], w[::-1])
    assert np.count_nonzero(_bits(rev) != _bits(ref)) >= n // 2
    assert ref[n - 1] == 0.0 and np.count_nonzero(e == 1) > 23000 and np.count_nonzero(e[:, 0] == e[:, 1]) >= 70
    ei = np.ascontiguousarray((e - 1).T.astype(np.int32))
    a, wv = (torch.from_numpy(ei).cuda(), torch.from_numpy(w).cuda()) if device else (ei, w)
    ctx.set_graph_view(a, wv, n=n, base=0)
    ctx.set_vertex_view(np.ones(n, dtype=np.int64))
    got = ctx.resident_graph()
    assert not got["unit"] and np.array_equal(_bits(got["vweight"]), _bits(ref))
    assert np.array_equal(_bits(ctx.vertex_weights()), _bits(ref))  # the public read-back: the same bits as the hook
    # fp32 weights: the fp64 form on the widened weights
    w32 = w.astype(np.float32)
    ref32 = _reference_vw(n, e, w32.astype(np.float64))
    ctx.set_graph_view(a, torch.from_numpy(w32).cuda() if device else w32, n=n, base=0)
    ctx.set_vertex_view(None)  # (the communities stay)
    assert np.array_equal(_bits(ctx.resident_graph()["vweight"]), _bits(ref32))
    assert np.count_nonzero(_bits(ref32) != _bits(ref)) >= n // 2


@pytest.mark.parametrize("n", [1, 64, 65, 100000])
def test_derived_vertex_weights_of_a_unit_list_are_the_degrees(ctx, n):
    import torch

    rng = np.random.default_rng(n)
    m = 5 if n == 1 else 40011
    e = rng.integers(1, n + 1, size=(m, 2)).astype(np.int64)
    e[::4, 1] = 1  # a hub
    e[1::7] = e[0]  # multi-edges
    e[2::500, 1] = e[2::500, 0]  # self-loops (counted twice)
    ref = np.bincount(e.ravel() - 1, minlength=n).astype(np.float64)
    assert np.array_equal(ref, _reference_vw(n, e, np.ones(m)))
    for weights in (None, np.ones(m, dtype=np.float32)):  # no weights, and weights that are all exactly 1.0
        a = torch.from_numpy(np.ascontiguousarray(e.T)).cuda()
        ctx.set_graph_view(a, None if weights is None else torch.from_numpy(weights).cuda(), n=n, base=1)
        ctx.set_vertex_view(torch.ones(n, dtype=torch.int32).cuda())
        got = ctx.resident_graph()
        assert got["unit"] and got["w"] is None and np.array_equal(_bits(got["vweight"]), _bits(ref))
        assert np.array_equal(_bits(ctx.vertex_weights()), _bits(ref))


# ---- 4. the vertex view -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=["int32", "int64"])
def test_vertex_view_builds_the_tables_of_set_vertex_data(ctx, dt, device):
    import torch

    from cge.jl_amd import api

    def held(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x).cuda() if device else x

    for n, C_ in ((1, 1), (65, 7), (40000, 300), (70000, 70000)):
        rng = np.random.default_rng(n)
        comm = rng.permutation(n).astype(np.int64) + 1 if C_ == n else rng.integers(1, C_ + 1, size=n).astype(np.int64)
        comm[0], comm[-1] = C_, 1  # the extrema occur
        if n == 1:
            comm[0] = 1
        vw = rng.random(n) + 0.5
        ctx.set_graph(np.array([[1, n]], dtype=np.int64), np.ones(1), n)
        ctx.set_vertex_data(comm, vw)
        ref = ctx.resident_graph()
        assert ref["n_comm_max"] == C_ and (ref["comm16"] is None) == (C_ >= 65536)
        if ref["comm16"] is not None:
            assert ref["comm16"].size % 32768 == 0 and ref["comm16"].size >= n
        for base in (0, 1, -1):
            ids = (comm - 1 + max(base, 0)).astype(dt)
            for vweights in (vw, vw.astype(np.float32), None):
                ctx.set_graph(np.array([[1, n]], dtype=np.int64), np.ones(1), n + 1)  # (another vertex set: the tables are dropped)
                ctx.set_graph(np.array([[1, n]], dtype=np.int64), np.ones(1), n)
                assert ctx.resident_graph()["comm"] is None
                ctx.set_vertex_view(held(ids), None if vweights is None else held(vweights), base=base)
                got = ctx.resident_graph()
                assert got["n_comm_max"] == C_ and np.array_equal(got["comm"], ref["comm"])
                assert (got["comm16"] is None) == (ref["comm16"] is None)
                if ref["comm16"] is not None:
                    assert np.array_equal(got["comm16"], ref["comm16"])
                if vweights is None:  # derived: the degrees of the one-edge graph
                    want = np.zeros(n)
                    np.add.at(want, [0, n - 1], 1.0)
                else:
                    want = vweights.astype(np.float64)
                assert np.array_equal(_bits(got["vweight"]), _bits(want))
    # a community id 0 after rebasing; a minimum that is neither 0 nor 1
    n = 65
    ctx.set_graph(np.array([[1, n]], dtype=np.int64), np.ones(1), n)
    ids = np.arange(n).astype(dt) % 5
    with pytest.raises(api.CGEError) as ei:
        ctx.set_vertex_view(held(ids), base=1)
    assert ei.value.code == -7 and "1-based" in str(ei.value)
    with pytest.raises(api.AssertionErrorCGE) as ei:
        ctx.set_vertex_view(held(ids + 2), base=-1)
    assert ei.value.code == -1 and "Communities should be either 0-based or 1-based" in str(ei.value)
    ctx.set_vertex_view(held(ids), base=0)
    assert ctx.resident_graph()["n_comm_max"] == 5


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
def _tensor_inputs(a, weighted):
    import torch

    ei = torch.from_numpy(np.ascontiguousarray((np.asarray(a["edges"]) - 1).T.astype(np.int32))).cuda()  # PyG's edge_index
    comm = torch.from_numpy(np.ascontiguousarray(np.asarray(a["comm"]).ravel() - 1)).cuda()
    w = torch.from_numpy(np.asarray(a["eweights"], dtype=np.float64)).cuda() if weighted else None
    return ei, comm, w


def _both_ways(ctx, a, weighted, **kw):
    from cge.jl_amd import api

    n = a["embedding"].shape[0]
    ctx.set_inputs(a["edges"], a["eweights"], a["vweights"], a["comm"], a["embedding"])
    ref = ctx.score(a["clusters"], a["land"], a["forced"], a["method"], **kw)
    ref_trace = ctx.last_trace
    split_ref = ctx.runsplit(a["clusters"], max(a["land"], 4), a["forced"], a["method"]) if a["land"] != -1 else None
    ei, comm, w = _tensor_inputs(a, weighted)
    ctx.set_graph(np.array([[1, 2]], dtype=np.int64), np.ones(1), n + 1)  # (nothing of the first way stays resident)
    assert ctx.set_graph_view(ei, w, n=n, base=0) == n
    ctx.set_vertex_view(comm, base=0)
    ctx.set_embedding(a["embedding"])
    assert np.array_equal(_bits(ctx.vertex_weights()), _bits(np.asarray(a["vweights"], dtype=np.float64)))  # parseargs' vweight
    got = ctx.score(api.FROM_COMM, a["land"], a["forced"], a["method"], **kw)
    assert np.array_equal(_bits(got), _bits(ref)), (got, ref)
    _same_trace(ctx.last_trace, ref_trace)
    if split_ref is not None:
        assert np.array_equal(ctx.runsplit(api.FROM_COMM, max(a["land"], 4), a["forced"], a["method"]), split_ref)
        N = ctx.landmarks_run(a["clusters"], a["land"], a["forced"], a["method"], kw.get("directed", False))
        assert ctx.landmarks_run(api.FROM_COMM, a["land"], a["forced"], a["method"], kw.get("directed", False)) == N
    return ref


@pytest.mark.parametrize("kw", [dict(seed=42, auc_samples=2000), dict(seed=-1, auc_samples=2000),
                                dict(seed=7, auc_samples=2000, directed=True, split=True)], ids=["seeded", "unseeded", "directed"])
@pytest.mark.parametrize("graph", ["test.edgelist", "test_weights.edgelist"])
def test_tensor_inputs_score_as_parseargs_arrays_test115(ctx, graph, kw):
    g = os.path.join(GOLDEN, "test115")
    weighted = graph != "test.edgelist"
    for land in ("20", None):  # landmark mode; exact mode (no -l: land = -1)
        argv = ["-g", f"{g}/{graph}", "-c", f"{g}/test1col.ecg", "-e", f"{g}/test_n2v.embedding", "-f", "1", "-m", "rss"]
        a = _parse(argv + (["-l", land] if land else []))
        assert (np.any(np.asarray(a["eweights"]) != 1.0)) == weighted
        _both_ways(ctx, a, weighted, **kw)


def test_tensor_call_gives_the_readme_answer_example10k(ctx, example10k):
    """README.md:88-100 from tensors: a 0-based int32 (2, m) edge_index and comm on the device, weights derived, clusters FROM_COMM,
    bit-equal to `set_inputs` + `score` on parseargs' arrays; then `score_tensors` on two embeddings of different dtype against
    `score_views`.  The README's known answer: element 1 exactly; element 2 has the bits of the array path, which
    tests/test_gpu_parity.py holds to the README's digits."""
    import torch

    from cge.jl_amd import api

    a = example10k
    kw = dict(seed=a["seed"], auc_samples=a["samples"])
    ref = _both_ways(ctx, a, False, **kw)
    assert ref[0] == 6.25 and ref[2] == 0.0 and ref[3] == 0.0
    assert abs(ref[1] - 0.002961243353776198) <= 1e-9 * 0.002961243353776198  # (the array path itself, as test_gpu_parity.py asks)
    emb = np.asarray(a["embedding"], dtype=np.float64)
    e32 = torch.from_numpy(emb.astype(np.float32)).cuda()
    members = [emb, e32]
    ctx.set_inputs(a["edges"], a["eweights"], a["vweights"], a["comm"], a["embedding"])
    want = ctx.score_views(members, a["clusters"], a["land"], a["forced"], a["method"], **kw)
    want_traces = ctx.last_traces
    ei, comm, _ = _tensor_inputs(a, False)
    got = api.score_tensors(ei, members, comm, a["land"], a["forced"], a["method"], base=0, ctx=ctx, **kw)
    assert len(got) == 2 and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got, want))
    for t, wt in zip(ctx.last_traces, want_traces):
        _same_trace(t, wt)
    assert np.array_equal(_bits(got[0]), _bits(ref))  # the fp64 member: the single score above
    one = api.score_tensors(ei.to(torch.int64).t().contiguous() + 1, e32, comm + 1, a["land"], a["forced"], a["method"], base=1, ctx=ctx,
                            **kw)
    assert np.array_equal(_bits(one), _bits(want[1]))  # (m, 2) int64 1-based ids, one embedding: a vector, not a list
