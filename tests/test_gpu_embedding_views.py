"""Embedding views on the GPU (`pytest -m gpu`): cge_set_embedding_view / cge_score_views take fp64 / fp32 / fp16 / bf16 embeddings
from host or device memory, row- or column-major, packed or with a leading dimension.  Widening to fp64 is exact, so the checks are
bitwise: the resident row-major matrix (cge_resident_embedding_test) holds the bits of `.astype(float64)` / `.to(torch.float64)`,
and every score, trace, diameter and landmark table is the one `set_embedding(widened array)` gives on the same context."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


# ---- 1. element-exact ingestion -------------------------------------------------------------------------------------------------
DTYPES = ("float64", "float32", "float16", "bfloat16")
SHAPES = ((1, 1), (31, 3), (33, 33), (65, 130), (1000, 16))
# bit patterns of +0, -0, the smallest subnormal (+/-), the largest finite value (+/-), +Inf, -Inf, a NaN
_BITS = {"float64": ("int64", 0, -2**63, 1, -2**63 + 1, 0x7FEFFFFFFFFFFFFF, -2**63 + 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000,
                     -2**63 + 0x7FF0000000000000, 0x7FF8000000000001),
         "float32": ("int32", 0, -2**31, 1, -2**31 + 1, 0x7F7FFFFF, -2**31 + 0x7F7FFFFF, 0x7F800000, -2**31 + 0x7F800000, 0x7FC00001),
         "float16": ("int16", 0, -2**15, 1, -2**15 + 1, 0x7BFF, -2**15 + 0x7BFF, 0x7C00, -2**15 + 0x7C00, 0x7E01),
         "bfloat16": ("int16", 0, -2**15, 1, -2**15 + 1, 0x7F7F, -2**15 + 0x7F7F, 0x7F80, -2**15 + 0x7F80, 0x7FC1)}


def _values(dtype, n, d, kind="finite", seed=0):
    """A packed (n, d) CPU tensor of `dtype`: normal values, with +/-0, the smallest subnormals and the largest finite values
    (kind "finite"), those and +/-Inf ("inf"), or those and a NaN ("nan") at the start -- as many of them as the matrix holds."""
    import torch

    t = getattr(torch, dtype)
    g = torch.Generator().manual_seed(seed + 1000 * n + d)
    x = (torch.randn(n * d, generator=g, dtype=torch.float64) * 3.0).to(t)
    bits = _BITS[dtype]
    pick = {"finite": bits[1:7], "inf": bits[7:9] + bits[1:7], "nan": bits[9:10] + bits[1:7]}[kind]
    special = torch.tensor(pick, dtype=getattr(torch, bits[0])).view(t)
    k = min(len(special), n * d)
    x[:k] = special[:k]
    return x.reshape(n, d)


def _widened(x):
    """The reference: the caller's own conversion to float64, as a C-order numpy array."""
    import torch

    w = x.to(torch.float64).contiguous().numpy()
    return w


def _laid_out(x, row_major, pad, device):
    """`x` (n, d) stored row- or column-major with `pad` extra elements in the leading dimension, on the host (numpy, or a torch
    CPU tensor for bfloat16) or on the GPU (a torch tensor)."""
    import torch

    n, d = x.shape
    if row_major:
        base = torch.zeros(n, d + pad, dtype=x.dtype)
        base[:, :d] = x
        if device:
            base = base.cuda()
        v = base[:, :d]
    else:
        base = torch.zeros(d, n + pad, dtype=x.dtype)
        base[:, :n] = x.t()
        if device:
            base = base.cuda()
        v = base[:, :n].t()
    assert v.shape == (n, d)
    if not device and x.dtype != torch.bfloat16:
        v = v.numpy()
    return v


def _graph_of(ctx, n):
    """A context accepts an embedding of the resident graph's vertex count only: a one-edge graph of n vertices."""
    if ctx.n != n:
        ctx.set_graph(np.array([[1, n]], dtype=np.int64), np.ones(1), n)


def _assert_resident(ctx, ref, ids=None):
    got, got_ids = ctx.resident_embedding()
    if ids is not None:
        assert np.array_equal(got_ids, ids)
    assert got.shape == ref.shape and got.dtype == np.float64
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))  # a NaN stays a NaN ...
    gb, rb = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)
    bad = np.flatnonzero((gb != rb) & ok)
    assert bad.size == 0, (bad[:8], got.ravel()[bad[:8]], ref.ravel()[bad[:8]])  # ... and everything else keeps its bits


@pytest.mark.parametrize("pad", [0, 5], ids=["packed", "ld+5"])
@pytest.mark.parametrize("row_major", [1, 0], ids=["rowmajor", "colmajor"])
@pytest.mark.parametrize("device", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_view_is_widened_element_exactly(ctx, dtype, device, row_major, pad):
    from cge.jl_amd import api

    for kind in ("finite", "inf"):
        for n, d in SHAPES:
            x = _values(dtype, n, d, kind)
            ref = _widened(x)
            if n * d >= 6:  # the reference conversion itself keeps the subnormals and the signed zeros
                sub = ref.ravel()[2 if kind == "finite" else 4]
                assert sub != 0.0 and abs(sub) < 1e-7
            src = _laid_out(x, row_major, pad, device)
            v, _ = api.embedding_view(src)
            assert v.on_device == device and v.dtype == DTYPES.index(dtype)
            if n > 1 and d > 1:
                assert v.row_major == row_major and v.ld == (d if row_major else n) + pad  # in place: the strides as they are
            _graph_of(ctx, n)
            ctx.set_embedding_view(src)
            assert ctx.d == d
            _assert_resident(ctx, ref, np.arange(n))


@pytest.mark.parametrize("dtype", DTYPES)
def test_view_whose_base_is_one_element_off_a_16_byte_boundary(ctx, dtype):
    """The slice X[:, 1:] of a tensor: aligned to its element and no more -- the kernels fall back to element-wise loads."""
    import torch

    for device in (0, 1):
        for row_major in (1, 0):
            for n, d in ((33, 33), (65, 130), (1000, 16)):
                x = _values(dtype, n, d)
                ref = _widened(x)
                flat = torch.zeros(n * d + 1, dtype=x.dtype)
                flat[1:] = (x if row_major else x.t()).reshape(-1)
                if device:
                    flat = flat.cuda()
                assert flat.data_ptr() % 16 == 0
                src = flat[1:].view(n, d) if row_major else flat[1:].view(d, n).t()
                assert src.data_ptr() % 16 == x.element_size()
                _graph_of(ctx, n)
                ctx.set_embedding_view(src)
                _assert_resident(ctx, ref)
    # ... and a column slice of a wider tensor, whose rows start at every alignment
    wide = _values(dtype, 65, 40).cuda()
    _graph_of(ctx, 65)
    ctx.set_embedding_view(wide[:, 1:])
    _assert_resident(ctx, _widened(wide[:, 1:].cpu()))
    # ... and an odd width at an aligned base and pitch: 16-byte loads, rows of the result that start 8 bytes off
    assert wide.data_ptr() % 16 == 0 and wide.stride(0) * wide.element_size() % 16 == 0
    ctx.set_embedding_view(wide[:, :33])
    _assert_resident(ctx, _widened(wide[:, :33].cpu()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_stays_a_nan_and_the_diameter_answers_nan(ctx, dtype):
    for device in (0, 1):
        for row_major in (1, 0):
            x = _values(dtype, 65, 130, "nan")
            ref = _widened(x)
            assert np.isnan(ref[0, 0]) and np.isnan(ref).sum() == 1
            _graph_of(ctx, 65)
            ctx.set_embedding_view(_laid_out(x, row_major, 5, device))
            _assert_resident(ctx, ref)
            hi, ai, aj = ctx.max_pair_dist()
            assert np.isnan(hi) and (ai, aj) == (1, 1)  # include/cge_hip.h: cge_max_pair_dist
    x = _values(dtype, 65, 130)
    x[0, :6] = 1.0  # (no extreme values: their distances overflow)
    ctx.set_embedding_view(_laid_out(x, 1, 0, 0))
    assert np.isfinite(ctx.max_pair_dist()[0])  # (the flag is per upload)


def test_a_device_view_of_host_memory_is_refused(ctx):
    from cge.jl_amd import api

    a = np.zeros((31, 3), dtype=np.float32)
    v, _ = api.embedding_view(a)
    v.on_device = 1
    _graph_of(ctx, 31)
    assert ctx.L.cge_set_embedding_view(ctx.h, C.byref(v), C.c_int64(31)) == -7
    assert b"not device memory" in ctx.L.cge_last_error(ctx.h)
    v.on_device, v.dtype = 0, 7
    assert ctx.L.cge_set_embedding_view(ctx.h, C.byref(v), C.c_int64(31)) == -7  # the boundary check runs first
    assert b"dtype" in ctx.L.cge_last_error(ctx.h)


# ---- 2. staging boundaries ------------------------------------------------------------------------------------------------------
def test_host_fp32_column_major_view_in_more_than_one_chunk(ctx):
    """70 000 x 256 fp32, column-major: 71.7 MB, more than one 64 MiB staging buffer -- whole columns per chunk, two chunks.
    The smallest shape of the issue that reaches the branch; 0.3 s on the MI355X."""
    n, d = 70_000, 256
    rng = np.random.default_rng(5)
    x = np.asfortranarray(rng.standard_normal((n, d), dtype=np.float32))
    assert x.nbytes > 64 << 20 and x.flags.f_contiguous
    _graph_of(ctx, n)
    ctx.set_embedding_view(x)
    _assert_resident(ctx, x.astype(np.float64))


def test_host_fp16_column_longer_than_a_staging_buffer(ctx):
    """(33 554 435, 2) fp16, column-major: one column is 6 bytes longer than a 64 MiB staging buffer, so every column goes up in
    row pieces.  Every finite fp16 bit pattern occurs.  The smallest shape that reaches the branch; it moves 134 MB up and
    fetches 537 MB of doubles back: 0.5 s on the MI355X."""
    n, d = 33_554_435, 2
    bits = (np.arange(n * d, dtype=np.uint32) % 0x7C00).astype(np.uint16)
    bits[1::2] |= 0x8000  # every other one negative
    x = bits.view(np.float16).reshape(d, n).T
    assert x.shape == (n, d) and x.strides == (2, 2 * n) and 2 * n > 64 << 20
    _graph_of(ctx, n)
    ctx.set_embedding_view(x)
    got, _ = ctx.resident_embedding()
    ref = x.astype(np.float64)
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(ref).view(np.uint64))


# ---- 2b. the fp64 entry points are views: cge_set_embedding / cge_set_embedding_device go through the same ingest -----------------
@pytest.mark.parametrize("form", ["set_embedding", "device_colmajor", "device_rowmajor"])
def test_fp64_entry_points_keep_the_callers_bits(ctx, form):
    """set_embedding (column-major host) and set_embedding_device (either layout) of float64: the resident matrix is the caller's
    array, bit for bit, at the shapes that straddle the 64 x 32 tile and the 16-byte vector edge."""
    import torch

    for kind in ("finite", "inf"):
        for n, d in SHAPES:
            x = _values("float64", n, d, kind)
            ref = x.numpy()
            _graph_of(ctx, n)
            if form == "set_embedding":
                ctx.set_embedding(ref)
            else:
                row_major = form == "device_rowmajor"
                t = (x if row_major else x.t()).contiguous().cuda()  # (d, n) C-order: the column-major (n, d) matrix
                torch.cuda.synchronize()
                ctx.set_embedding_device(t.data_ptr(), n, d, row_major=row_major)
            assert ctx.d == d
            _assert_resident(ctx, ref, np.arange(n))


def test_host_fp64_column_major_matrix_in_more_than_one_chunk(ctx):
    """set_embedding of 70 000 x 128 float64: 71.68 MB against a 64 MiB staging buffer -- 119 whole columns fit a chunk, two chunks.
    The smallest d = 128 shape that reaches the branch."""
    n, d = 70_000, 128
    x = np.asfortranarray(np.random.default_rng(6).standard_normal((n, d)))
    assert x.nbytes > 64 << 20 and (64 << 20) // (8 * n) == 119 and x.flags.f_contiguous
    _graph_of(ctx, n)
    ctx.set_embedding(x)
    _assert_resident(ctx, np.ascontiguousarray(x))


def test_host_fp64_column_longer_than_a_staging_buffer(ctx):
    """set_embedding of (8 388 609, 2) float64: one column is 8 bytes longer than a 64 MiB staging buffer, so every column goes up
    in row pieces.  134 MB up, 134 MB back.  The bit patterns: a counter times an odd constant, the top exponent bit cleared (so
    every value is finite), both signs."""
    n, d = 8_388_609, 2
    bits = (np.arange(n * d, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xBFFFFFFFFFFFFFFF)
    x = bits.view(np.float64).reshape(d, n).T
    assert x.shape == (n, d) and x.strides == (8, 8 * n) and 8 * n == (64 << 20) + 8
    _graph_of(ctx, n)
    ctx.set_embedding(x)
    _assert_resident(ctx, np.ascontiguousarray(x))


def test_a_host_pointer_handed_to_set_embedding_device_is_refused(ctx):
    a = np.asfortranarray(_values("float64", 31, 3).numpy())
    _graph_of(ctx, 31)
    rc = ctx.L.cge_set_embedding_device(ctx.h, C.c_void_p(a.ctypes.data), C.c_int64(31), C.c_int64(3), C.c_int(0))
    assert rc == -7  # CGE_E_ARG: the pointer's attributes are asked for, nothing is dereferenced
    err = ctx.L.cge_last_error(ctx.h)
    assert b"not device memory" in err and b"set_embedding_device" in err
    ctx.set_embedding(a)  # the context is as usable as before
    _assert_resident(ctx, np.ascontiguousarray(a), np.arange(31))


# ---- 3. results follow ----------------------------------------------------------------------------------------------------------
def _scored(ctx, g, **kw):
    res = ctx.score(g["clusters"], 400, seed=5, auc_samples=6000, **kw)
    return res, ctx.last_trace, ctx.get_stat("diameter_bits"), ctx.landmarks_fetch()


def _assert_same_score(got, exp):
    assert np.array_equal(got[0], exp[0]), (got[0], exp[0])
    assert got[1]["n_alpha"] == exp[1]["n_alpha"] and got[1]["iters"] == exp[1]["iters"]
    assert np.array_equal(got[1]["div"], exp[1]["div"], equal_nan=True) and np.array_equal(got[1]["auc"], exp[1]["auc"], equal_nan=True)
    assert got[2] == exp[2]  # the diameter's bits
    for a, b in zip(got[3], exp[3]):  # d_ii, centroids, communities, landmark edges, weights, landmark weights, v_to_l
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_scores_after_a_view_are_those_of_the_widened_array(ctx):
    import torch
    from test_gpu_batch import _case, _setup

    g, ew, vw = _case()
    _setup(ctx, g, ew, vw)
    x32 = np.ascontiguousarray(np.asarray(g["embedding"]), dtype=np.float32)  # C order
    ctx.set_embedding(x32.astype(np.float64))
    exp32 = _scored(ctx, g)
    xb = torch.from_numpy(x32).to(torch.bfloat16)
    ctx.set_embedding(xb.to(torch.float64).numpy())
    expb = _scored(ctx, g)
    assert not np.array_equal(exp32[0], expb[0])  # (the rounding to bf16 is a different embedding)
    wide = torch.zeros(g["n"], 24, dtype=torch.float32, device="cuda")
    wide[:, 4:20] = torch.from_numpy(x32).cuda()
    for src, exp in ((x32, exp32), (torch.from_numpy(x32).cuda(), exp32), (xb.cuda(), expb), (wide[:, 4:20], exp32)):
        ctx.set_embedding_view(src)
        _assert_same_score(_scored(ctx, g), exp)


# ---- 4. score_views equals separate scores --------------------------------------------------------------------------------------
def _members(g, d_small, seed):
    """Four members of one graph: float64 F-order host, float32 C-order host, a bf16 CUDA tensor, a float32 CUDA slice of the
    first `d_small` columns -- and the float64 arrays they widen to."""
    import torch

    rng = np.random.default_rng(seed)
    X = np.asarray(g["embedding"])
    m0 = np.asfortranarray(X)
    m1 = np.ascontiguousarray(X + 0.4 * rng.standard_normal(X.shape), dtype=np.float32)
    m2 = torch.from_numpy(X + 0.8 * rng.standard_normal(X.shape)).to(torch.bfloat16).cuda()
    m3 = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()[:, :d_small]
    assert m3.stride() == (X.shape[1], 1) and m3.shape[1] == d_small < X.shape[1]
    wid = [m0, m1.astype(np.float64), m2.cpu().to(torch.float64).numpy(), m3.cpu().to(torch.float64).numpy()]
    return [m0, m1, m2, m3], wid


def test_score_views_of_four_different_members_equals_separate_scores(ctx):
    from test_gpu_batch import _assert_same, _case, _separate, _setup

    g, ew, vw = _case()
    _setup(ctx, g, ew, vw)
    members, wid = _members(g, 8, seed=1)
    kw = dict(forced=4, method="rss", seed=5, auc_samples=6000)
    got = ctx.score_views(members, g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    launches, alphas = ctx.get_stat("fit_batched_launches"), ctx.get_stat("fit_batched_alphas")
    assert ctx.d == 8
    _assert_resident(ctx, wid[3])  # afterwards the last member is the resident one
    exp, exp_tr = _separate(ctx, wid, g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)
    n_alpha = [t["n_alpha"] for t in exp_tr]
    assert alphas == sum(n_alpha)  # every member-alpha was fitted by a shared launch ...
    assert launches < sum(n_alpha)  # ... and the launches really were shared
    # the narrow member first: nothing kept between members is sized by the member before it
    got = ctx.score_views(members[::-1], g["clusters"], 400, **kw)
    _assert_same(got, ctx.last_traces, exp[::-1], exp_tr[::-1])
    _assert_resident(ctx, wid[0])


def test_directed_score_views_equals_separate_scores(ctx):
    from cge.jl_amd import synth
    from test_gpu_batch import _assert_same, _separate

    g = synth.abcd_like(3000, 24000, 6, 8, seed=3, directed=True)
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    members, wid = _members(g, 4, seed=5)
    kw = dict(forced=4, method="rss", directed=True, seed=2, auc_samples=4000)
    got = ctx.score_views(members, g["clusters"], 100, **kw)
    got_tr = ctx.last_traces
    assert ctx.get_stat("fit_batched_launches") == 0  # (the directed sweep is not batched: members one after another)
    _assert_resident(ctx, wid[3])
    exp, exp_tr = _separate(ctx, wid, g["clusters"], 100, **kw)
    _assert_same(got, got_tr, exp, exp_tr)


def test_score_views_with_a_homogeneous_member_returns_its_error_and_leaves_the_context_usable(ctx):
    from cge.jl_amd import api
    from test_gpu_batch import _assert_same, _case, _separate

    g, ew, _ = _case()
    n, d = g["n"], g["embedding"].shape[1]
    ctx.set_graph(g["edges"], ew, n)
    ctx.set_vertex_data(g["comm"], np.full(n, 2.0))
    bad = np.tile(np.arange(1.0, d + 1.0, dtype=np.float32), (n, 1))  # all rows equal
    members, wid = _members(g, 8, seed=6)
    kw = dict(forced=4, method="rss", seed=1, auc_samples=5000)
    # the C entry point itself: the member's status, every out_len 0
    srcs = [members[1], bad, members[3]]
    views, keep = (api.EmbeddingView * 3)(), []
    for k, s in enumerate(srcs):
        views[k], owner = ctx._view(s)
        keep.append(owner)
    flat, off = api._flatten_clusters(g["clusters"])
    a = api.ScoreArgs()
    a.clusters_flat, a.clusters_off, a.n_clusters = flat.ctypes.data, off.ctypes.data, len(off) - 1
    a.land, a.forced, a.method, a.seed, a.auc_samples = 400, 4, 0, 1, 5000
    out, olen = np.zeros((3, 7)), (C.c_int * 3)(7, 7, 7)
    rc = ctx.L.cge_score_views(ctx.h, C.byref(a), views, C.c_int64(3), out.ctypes.data_as(C.c_void_p), olen, None)
    assert rc == -2 and list(olen) == [0, 0, 0]  # CGE_E_HOMOGENEOUS
    with pytest.raises(api.CGEError, match="homogenous"):
        ctx.score_views([bad] + members[:2], g["clusters"], 400, **kw)
    assert len(ctx.draw_samples(1, 5000)[0]) == 5000
    got = ctx.score_views(members[:3], g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    assert ctx.get_stat("fit_batched_alphas") > 0
    exp, exp_tr = _separate(ctx, wid[:3], g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)


def test_score_views_checks_its_members(ctx):
    import torch
    from cge.jl_amd import api
    from test_gpu_batch import _case, _setup

    g, ew, vw = _case()
    _setup(ctx, g, ew, vw)
    with pytest.raises(ValueError):
        ctx.score_views([np.zeros((g["n"] - 1, 4), dtype=np.float32)], g["clusters"], 400)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ctx.set_embedding_view(torch.zeros(g["n"], 4, device="cuda:1"))
    ctx.set_option("shard_ingest", 1)  # not under sharding, as the batch
    try:
        with pytest.raises(api.CGEError, match="sharding"):
            ctx.score_views([np.asarray(g["embedding"], dtype=np.float32)], g["clusters"], 400)
    finally:
        ctx.set_option("shard_ingest", 0)


# ---- 5. two ranks on one GPU ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _graph_two_ranks():
    from cge.jl_amd import synth

    return synth.abcd_like(20000, 200000, 20, 16, seed=21)


def _source_two_ranks(g, case):
    """(the view's source on the host, the float64 array it widens to)"""
    X = np.asarray(g["embedding"])
    if case.endswith("f16_colmajor_host"):
        src = np.asfortranarray(X.astype(np.float16))
    else:
        src = np.ascontiguousarray(X, dtype=np.float32)
    return src, np.asfortranarray(src.astype(np.float64))


SCORE_KW = dict(seed=5, auc_samples=4000)


def _rank_views(rank, world, port, q, case):
    try:
        import torch
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from cge.jl_amd import api
        from cge.jl_amd.dist import TorchCollectives

        g = _graph_two_ranks()
        src, wid = _source_two_ranks(g, case)
        if case == "rows_f32_cuda":
            src = torch.from_numpy(src).cuda()
        ctx = api.Context(0)
        coll = TorchCollectives(ctx, 600 * 600 * 2 + 1024, torch.device("cuda", 0))  # collectives first: the uploads are split
        ctx.set_option("shard_ingest", 1)
        ctx.set_option("shard_rows", 0 if case.startswith("ingest") else 1)
        ctx.set_graph(g["edges"], g["eweights"], g["n"])
        ctx.set_vertex_data(g["comm"], g["vweights"])
        ctx.set_option("fit_persistent", 1)  # (two processes cannot both keep a persistent grid resident on one GPU)
        ctx.set_embedding(wid)  # the fp64 form under the same options ...
        ref = ctx.score(g["clusters"], 400, 2, "rss", **SCORE_KW)
        ref_hi = ctx.get_stat("diameter_bits")
        ctx.set_embedding_view(src)  # ... and the view
        rows, ids = ctx.resident_embedding()
        exact = bool(np.array_equal(rows.view(np.uint64), np.ascontiguousarray(wid[ids]).view(np.uint64)))
        stats = (ctx.get_stat("rows_resident"), ctx.get_stat("rows_total"), int(rows.shape[0]), int(rows.shape[1]))
        res = ctx.score(g["clusters"], 400, 2, "rss", **SCORE_KW)
        q.put((rank, res.tolist(), ref.tolist(), exact, stats, ids.tolist(), (ctx.get_stat("diameter_bits"), ref_hi)))
        ctx.close()
        del coll
    except Exception as e:  # surface the failure in the parent
        import traceback

        q.put((rank, traceback.format_exc() + repr(e), None, None, None, None, None))
    finally:
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("case", ["rows_f32_rowmajor_host", "rows_f16_colmajor_host", "rows_f32_cuda", "ingest_f16_colmajor_host"])
def test_two_ranks_take_views(ctx, case):
    """shard_rows: a rank uploads (host view) or gathers (CUDA tensor) the rows of its own communities only, in the view's type;
    shard_ingest: a rank uploads its n / 2 rows of an fp16 column-major view and the widened pieces are all-gathered.  Each rank's
    resident rows are the widened matrix's, by the ids the hook returns, and its score is the one the fp64 form gives under the
    same options -- and the one-rank score of the widened array."""
    import queue

    import torch.multiprocessing as mp

    g = _graph_two_ranks()
    _, wid = _source_two_ranks(g, case)
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    ctx.set_embedding(wid)
    try:
        ctx.set_option("fit_persistent", 1)
        one = ctx.score(g["clusters"], 400, 2, "rss", **SCORE_KW)
        one_hi = ctx.get_stat("diameter_bits")
    finally:
        ctx.set_option("fit_persistent", 0)
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_rank_views, args=(r, 2, port, q, case)) for r in range(2)]
    for p in procs:
        p.start()
    results = []
    try:
        for _ in procs:
            results.append(q.get(timeout=300))  # (each rank's GPU work under its own limit; nothing is started after a failure)
            assert results[-1][3] is not None, results[-1][1]  # a traceback otherwise
    except queue.Empty:
        pytest.fail("a rank did not answer in time")
    finally:
        for p in procs:
            p.join(10 if len(results) < 2 else 120)
            if p.is_alive():
                p.kill()
    held = []
    for rank, res, ref, exact, stats, ids, hi in sorted(results):
        resident, total, r, d = stats
        assert exact, f"rank {rank}: the resident rows are not the widened view's"
        assert total == g["n"] and d == 16 and r == len(ids)
        if case.startswith("rows"):
            assert resident == r and 0.35 * total < resident < 0.65 * total  # about n / 2 rows in HBM
            held += ids
        else:
            assert ids == list(range(g["n"]))  # (ingest sharding: every rank ends with every row)
        assert res == ref and hi[0] == hi[1]  # the bits of the fp64 form under the same options
        assert hi[0] == one_hi
        assert res[0] == one[0] and res[4] == one[4]
        # Against the ONE-rank score the comparison is the one test_gpu_two_ranks.py makes for the fp64 forms: two ranks group the
        # sums of the sweep differently from one (include/cge_hip.h, "shard_samples": last-bit differences of elements 5-7), so
        # bitwise equality does not hold between one and two ranks for ANY form of upload.  What the view must not change is
        # checked bitwise just above: `res == ref`, the fp64 form's score under the same two-rank options.
        assert np.allclose(res, one, rtol=1e-12, atol=1e-14), (rank, res, one)
    if case.startswith("rows"):
        assert sorted(held) == list(range(g["n"]))  # every row is resident on exactly one rank
    assert results[0][1] == results[1][1]  # both ranks hold the same bits


# ---- 6. cge_compare.py ----------------------------------------------------------------------------------------------------------
def test_compare_script_takes_npy_files_of_different_dtype_and_width(tmp_path):
    g = os.path.join(GOLDEN, "example10k")
    emb = np.loadtxt(os.path.join(g, "10k.embedding"))
    emb = emb[np.argsort(emb[:, 0].astype(np.int64), kind="stable")]
    ids, x32 = emb[:, :1], np.ascontiguousarray(emb[:, 1:], dtype=np.float32)
    x16 = np.ascontiguousarray(x32[:, : x32.shape[1] // 2], dtype=np.float16)
    f32_npy, f16_npy = os.path.join(tmp_path, "a32.npy"), os.path.join(tmp_path, "b16.npy")
    f32_txt, f16_txt = os.path.join(tmp_path, "a32.embedding"), os.path.join(tmp_path, "b16.embedding")
    np.save(f32_npy, x32)
    np.save(f16_npy, x16)
    for path, x in ((f32_txt, x32), (f16_txt, x16)):
        np.savetxt(path, np.hstack([ids, x.astype(np.float64)]), fmt=["%d"] + ["%.17g"] * x.shape[1])
    flags = ["-g", f"{g}/10k.edgelist", "-c", f"{g}/10k.ecg", "-l", "400", "--seed", "42"]
    env = dict(os.environ)
    cmp_ = subprocess.run([sys.executable, os.path.join(ROOT, "cge_compare.py"), *flags, "-e", f32_npy, "-e", f16_npy, "-e", f32_txt],
                          capture_output=True, text=True, timeout=300, env=env)
    assert cmp_.returncode == 0, cmp_.stderr[-2000:]
    lines = cmp_.stdout.strip().split("\n")
    assert len(lines) == 3
    names, vecs = zip(*(ln.split("\t") for ln in lines))
    assert list(names) == [f32_npy, f16_npy, f32_txt]
    assert vecs[0] == vecs[2] and vecs[1] != vecs[0]  # the .npy float32 line is the text line, character for character
    for txt, vec in ((f32_txt, vecs[0]), (f16_txt, vecs[1])):  # ... and each is cge_cli.py's output for that embedding alone
        cli = subprocess.run([sys.executable, os.path.join(ROOT, "cge_cli.py"), *flags, "-e", txt],
                             capture_output=True, text=True, timeout=300, env=env)
        assert cli.returncode == 0, cli.stderr[-2000:]
        assert cli.stdout.strip() == vec
