"""CPU tests of the graph views (cge_graph_view / cge_vertex_view): the boundary check refuses what it must without a context or a
GPU, `api.graph_view` / `api.vertex_view` describe numpy arrays where they lie -- no copy -- or pack them once, and the clusters that
`FROM_COMM` stands for (restated in pure Python, `api.clusters_of`) are parseargs' clusters on both golden fixtures.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _lib():
    from cge.jl_amd import api

    L = api.load_library()
    L.cge_graph_view_check.restype = C.c_int
    L.cge_graph_view_check.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]
    return L


def _gv(src, dst, stride=1, id_dtype=0, base=-1, w=None, w_dtype=0, on_device=0):
    from cge.jl_amd import api

    g = api.GraphView()
    g.src, g.dst, g.stride, g.id_dtype, g.base, g.w, g.w_dtype, g.on_device = src, dst, stride, id_dtype, base, w, w_dtype, on_device
    return g


def _check(g, m):
    err = C.create_string_buffer(256)
    rc = _lib().cge_graph_view_check(C.byref(g) if g is not None else None, m, err, 256)
    return rc, err.value.decode()


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    thdr = open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    assert "int cge_graph_view_check(const cge_graph_view *g, int64_t m, char *err, int64_t err_len);" in hdr
    assert re.search(r"int cge_set_graph_view\(cge_ctx \*ctx, const cge_graph_view \*g, int64_t m, int64_t n [^;]*, int64_t \*n_out\);", hdr)
    assert "int cge_set_vertex_view(cge_ctx *ctx, const cge_vertex_view *v, int64_t n);" in hdr
    assert "int cge_vertex_weights(cge_ctx *ctx, double *out, int64_t n);" in hdr
    assert "} cge_graph_view;" in hdr and "} cge_vertex_view;" in hdr
    assert re.search(r"#define CGE_ID_I64 0\b", hdr) and re.search(r"#define CGE_ID_I32 1\b", hdr)
    assert "#define CGE_ABI_VERSION 1" in hdr  # additions only: the ABI version stays
    assert "int cge_resident_graph_test(void *ctx, cge_resident_graph *out);" in thdr
    L = _lib()
    for sym in ("cge_graph_view_check", "cge_set_graph_view", "cge_set_vertex_view", "cge_vertex_weights", "cge_resident_graph_test"):
        assert hasattr(L, sym), sym
    assert L.cge_abi_version() == 1


def test_struct_mirrors_have_the_c_layout():
    from cge.jl_amd import api

    assert C.sizeof(api.GraphView) == 48 and api.GraphView.w.offset == 32 and api.GraphView.on_device.offset == 44
    assert C.sizeof(api.VertexView) == 32 and api.VertexView.vweights.offset == 16
    assert C.sizeof(api.ResidentGraph) == 4 * 8 + 2 * 4 + 6 * 8 + 3 * 8


def test_null_context_fails_at_the_boundary():
    from cge.jl_amd import api

    L = _lib()
    a = np.zeros(8, dtype=np.int64)
    g = _gv(a.ctypes.data, a.ctypes.data + 32)
    v = api.VertexView()
    assert L.cge_set_graph_view(None, C.byref(g), C.c_int64(4), C.c_int64(0), None) == -7
    assert L.cge_set_vertex_view(None, C.byref(v), C.c_int64(4)) == -7
    assert L.cge_vertex_weights(None, a.ctypes.data_as(C.c_void_p), C.c_int64(4)) == -7
    assert L.cge_resident_graph_test(None, C.byref(api.ResidentGraph())) == -7


def test_graph_view_check_refuses_malformed_views():
    a = np.zeros(64, dtype=np.int64)
    w = np.zeros(16, dtype=np.float64)
    p, m = a.ctypes.data, 8
    good = lambda **kw: _gv(p, p + 8 * m, **kw)  # noqa: E731
    assert _check(good(), m) == (0, "")
    assert _check(None, m)[0] == -7
    assert _check(_gv(None, p), m)[0] == -7 and _check(_gv(p, None), m)[0] == -7  # NULL pointers
    assert _check(good(), 0)[0] == -7 and _check(good(), -3)[0] == -7  # m <= 0
    assert _check(good(stride=0), m)[0] == -7 and _check(good(stride=-1), m)[0] == -7  # stride < 1
    assert _check(good(id_dtype=2), m)[0] == -7 and _check(good(id_dtype=-1), m)[0] == -7  # unknown id dtype
    assert _check(good(base=2), m)[0] == -7 and _check(good(base=-2), m)[0] == -7
    for wd in (2, 3, 4, -1):  # F16, BF16 and unknown weight dtypes
        rc, msg = _check(good(w=w.ctypes.data, w_dtype=wd), m)
        assert rc == -7 and "weights" in msg
    assert _check(good(w=w.ctypes.data, w_dtype=2), m)[0] == -7
    assert _check(good(w=None, w_dtype=3), m)[0] == 0  # no weights: their dtype is not looked at
    rc, msg = _check(_gv(p + 4, p + 8 * m), m)  # an int64 pointer on a 4-byte boundary
    assert rc == -7 and "aligned" in msg
    assert _check(_gv(p, p + 8 * m + 2), m)[0] == -7
    assert _check(_gv(p + 2, p + 4 * m, id_dtype=1), m)[0] == -7  # int32 on a 2-byte boundary
    assert _check(good(w=w.ctypes.data + 4, w_dtype=0), m)[0] == -7 and _check(good(w=w.ctypes.data + 4, w_dtype=1), m)[0] == 0
    # dst overlapping src in a way the stride does not explain
    rc, msg = _check(_gv(p, p), m)  # the same column twice
    assert rc == -7 and "overlap" in msg
    assert _check(_gv(p, p + 8 * (m - 1)), m)[0] == -7  # two stride-1 columns, one element short of disjoint
    assert _check(_gv(p, p + 8 * 4, stride=2), m)[0] == -7  # stride 2: dst starts on an element of src
    assert _check(_gv(p, p + 8 * 3, stride=2), m)[0] == -7  # ... or further in than the stride reaches
    assert _check(_gv(p + 8 * 2, p, stride=2), m)[0] == -7
    # every refusal comes with a message; err may be NULL
    assert all(_check(g, m)[1] for g in (_gv(None, p), good(stride=0), good(id_dtype=5), _gv(p, p)))
    assert _lib().cge_graph_view_check(C.byref(good(stride=0)), m, None, 0) == -7


@pytest.mark.parametrize("id_dtype", [0, 1])
@pytest.mark.parametrize("on_device", [0, 1])
def test_graph_view_check_accepts_well_formed_views(id_dtype, on_device):
    a = np.zeros(256, dtype=np.int64)
    w = np.zeros(16)
    p, m, es = a.ctypes.data, 8, (8, 4)[id_dtype]
    for base in (-1, 0, 1):
        assert _check(_gv(p, p + es * m, 1, id_dtype, base, on_device=on_device), m) == (0, "")  # the rows of a (2, m) array
    assert _check(_gv(p, p + es, 2, id_dtype), m)[0] == 0  # an (m, 2) C-order array
    assert _check(_gv(p + es, p, 2, id_dtype), m)[0] == 0  # ... with its columns swapped
    assert _check(_gv(p, p + 2 * es, 3, id_dtype), m)[0] == 0  # columns 0 and 2 of an (m, 3) array
    assert _check(_gv(p + es, p + es * (m + 2), 1, id_dtype), m)[0] == 0  # a slice [:, 1:]: aligned to the element, no more
    assert _check(_gv(p + es * 100, p, 1, id_dtype), m)[0] == 0  # dst before src
    assert _check(_gv(p, p + es, 1, id_dtype), 1)[0] == 0  # one edge
    for wd in (0, 1):
        assert _check(_gv(p, p + es * m, 1, id_dtype, w=w.ctypes.data, w_dtype=wd), m)[0] == 0


# ---- api.graph_view / api.vertex_view -----------------------------------------------------------------------------------------------
def _form(g, a):
    """(src offset, dst offset from src, stride) in elements of the array `a` the view must point into."""
    sz = a.dtype.itemsize
    return (g.src - a.ctypes.data) // sz, (g.dst - g.src) // sz, g.stride


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_graph_view_of_numpy_arrays_in_place(dt):
    from cge.jl_amd import api

    m = 11
    code = api.ID_I32 if dt == np.int32 else api.ID_I64
    ei = np.arange(2 * m, dtype=dt).reshape(2, m)  # (2, m), C order: two rows
    g, keep, mm = api.graph_view(ei)
    assert keep[0] is ei and mm == m and _form(g, ei) == (0, m, 1) and (g.id_dtype, g.base, g.on_device, g.w) == (code, -1, 0, None)
    e2 = np.ascontiguousarray(ei.T)  # (m, 2), C order: interleaved pairs
    g, keep, mm = api.graph_view(e2, base=0)
    assert keep[0] is e2 and mm == m and _form(g, e2) == (0, 1, 2) and g.base == 0
    g, keep, mm = api.graph_view(ei.T)  # (m, 2) as the transpose of (2, m): F order
    assert mm == m and g.src == ei.ctypes.data and _form(g, ei) == (0, m, 1)
    f = np.asfortranarray(ei)  # (2, m), F order: the pairs are interleaved
    g, keep, mm = api.graph_view(f)
    assert keep[0] is f and mm == m and _form(g, f) == (0, 1, 2)
    s = ei[:, 1:]  # a slice: element-aligned
    g, keep, mm = api.graph_view(s, base=1)
    assert mm == m - 1 and _form(g, ei) == (1, m, 1)
    s = ei[:, ::3]  # a regular step
    g, keep, mm = api.graph_view(s)
    assert mm == 4 and _form(g, ei) == (0, m, 3)
    s = ei[::-1]  # the rows swapped: dst lies before src
    g, keep, mm = api.graph_view(s)
    assert mm == m and _form(g, ei) == (m, -m, 1)
    wide = np.arange(3 * m, dtype=dt).reshape(m, 3)  # columns 0 and 2 of an (m, 3) table
    g, keep, mm = api.graph_view(wide[:, ::2])
    assert mm == m and _form(g, wide) == (0, 2, 3)
    one = np.array([[4], [7]], dtype=dt)  # a single edge
    g, keep, mm = api.graph_view(one)
    assert mm == 1 and g.stride == 1 and g.dst - g.src == one.dtype.itemsize
    for arr in (ei, e2, f, ei[:, 1:], wide[:, ::2]):  # ... and the library's own check accepts every one of them
        g, keep, mm = api.graph_view(arr)
        assert _check(g, mm) == (0, "")


def test_graph_view_packs_once_when_no_stride_form_fits():
    from cge.jl_amd import api

    m = 9
    ei = np.arange(2 * m, dtype=np.int32).reshape(2, m)
    g, keep, mm = api.graph_view(ei[:, ::-1])  # a negative step: one packed copy in the same dtype
    assert keep[0] is not ei and keep[0].dtype == np.int32 and np.array_equal(keep[0], ei[:, ::-1])
    assert g.src == keep[0].ctypes.data and _form(g, keep[0]) == (0, m, 1) and g.id_dtype == api.ID_I32
    for other in (np.int16, np.uint8, np.float64):  # other dtypes become int64
        g, keep, mm = api.graph_view(ei.astype(other))
        assert keep[0].dtype == np.int64 and g.id_dtype == api.ID_I64 and np.array_equal(keep[0], ei)
    g, keep, mm = api.graph_view([[1, 2, 3], [2, 3, 1]])  # a list of lists
    assert mm == 3 and g.id_dtype == api.ID_I64
    with pytest.raises(ValueError):
        api.graph_view(np.zeros((3, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        api.graph_view(np.zeros((2, 0), dtype=np.int64))
    with pytest.raises(TypeError):
        api.graph_view(12345)


def test_graph_view_weights():
    from cge.jl_amd import api

    m = 6
    ei = np.arange(2 * m, dtype=np.int64).reshape(2, m)
    w64, w32 = np.linspace(1, 2, m), np.linspace(1, 2, m).astype(np.float32)
    g, keep, _ = api.graph_view(ei, w64)
    assert g.w == w64.ctypes.data and g.w_dtype == api.DTYPE_F64 and keep[1] is w64
    g, keep, _ = api.graph_view(ei, w32)
    assert g.w == w32.ctypes.data and g.w_dtype == api.DTYPE_F32
    g, keep, _ = api.graph_view(ei, w32.astype(np.float16))  # fp16 weights are not a view's: widened to float64 here
    assert g.w_dtype == api.DTYPE_F64 and keep[1].dtype == np.float64 and np.array_equal(keep[1], w32.astype(np.float16).astype(np.float64))
    wide = np.ones((m, 2))
    g, keep, _ = api.graph_view(ei, wide[:, 0])  # a strided column: packed once
    assert keep[1] is not wide and keep[1].flags.c_contiguous and g.w == keep[1].ctypes.data
    with pytest.raises(ValueError):
        api.graph_view(ei, np.ones(m + 1))
    assert _check(g, m) == (0, "")


def test_graph_view_of_torch_tensors():
    import torch

    from cge.jl_amd import api

    m = 7
    t = torch.arange(2 * m, dtype=torch.int32).reshape(2, m)
    g, keep, mm = api.graph_view(t)
    assert mm == m and g.src == t.data_ptr() and g.dst == t.data_ptr() + 4 * m and (g.stride, g.id_dtype, g.on_device) == (1, api.ID_I32, 0)
    g, keep, mm = api.graph_view(t[:, 1:])
    assert mm == m - 1 and g.src == t.data_ptr() + 4 and g.dst - g.src == 4 * m
    g, keep, mm = api.graph_view(t.t().contiguous().to(torch.int64))
    assert mm == m and (g.stride, g.id_dtype) == (2, api.ID_I64) and g.dst - g.src == 8
    g, keep, mm = api.graph_view(t.to(torch.int16))
    assert keep[0].dtype == torch.int64 and g.id_dtype == api.ID_I64
    g, keep, mm = api.graph_view(t, torch.ones(m, dtype=torch.float32))
    assert g.w_dtype == api.DTYPE_F32 and g.w == keep[1].data_ptr()


def test_vertex_view_descriptors():
    from cge.jl_amd import api

    n = 10
    c64, c32 = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int32)
    v, keep, nn = api.vertex_view(c64)
    assert nn == n and v.comm == c64.ctypes.data and (v.id_dtype, v.base, v.vweights, v.on_device) == (api.ID_I64, -1, None, 0)
    v, keep, nn = api.vertex_view(c32.reshape(n, 1), base=0)  # comm::Matrix{Int} n x 1
    assert nn == n and v.comm == c32.ctypes.data and (v.id_dtype, v.base) == (api.ID_I32, 0)
    v, keep, nn = api.vertex_view(np.arange(2 * n, dtype=np.int64)[::2])  # strided: packed once, same dtype
    assert nn == n and keep[0].flags.c_contiguous and keep[0].dtype == np.int64 and v.comm == keep[0].ctypes.data
    vw = np.linspace(0, 1, n).astype(np.float32)
    v, keep, nn = api.vertex_view(c64, vw, base=1)
    assert v.vweights == vw.ctypes.data and v.vw_dtype == api.DTYPE_F32
    v, keep, nn = api.vertex_view(None, np.ones(n))
    assert nn == n and v.comm is None and v.vw_dtype == api.DTYPE_F64
    with pytest.raises(ValueError):
        api.vertex_view(c64, np.ones(n + 1))


# ---- clusters from communities ----------------------------------------------------------------------------------------------------
def _canon(clusters):
    return sorted(tuple(int(x) for x in c) for c in clusters)


@pytest.mark.parametrize("fixture", ["test115", "example10k"])
def test_clusters_of_comm_are_parseargs_clusters(fixture, request):
    """What FROM_COMM stands for (src/auxilary.jl:199-208), restated in pure Python, against parseargs on the golden fixtures:
    the same clusters with the same members in the same (ascending) order; only the order of the clusters is free (the reference
    collects the values of a Dict, and runsplit sorts them)."""
    from cge.jl_amd import api

    a = request.getfixturevalue(fixture)
    comm = np.asarray(a["comm"]).ravel()
    mine = api.clusters_of(comm)
    assert _canon(mine) == _canon(a["clusters"])
    assert sum(len(c) for c in mine) == len(comm) and len(mine) == len(np.unique(comm))
    assert all(np.all(np.diff(c) > 0) for c in mine) and all(len(c) for c in mine)
    assert _canon(api.clusters_of(comm - 1)) == _canon(mine)  # ids are labels: 0-based communities give the same clusters


def test_from_comm_maps_to_minus_one():
    from cge.jl_amd import api

    assert api._cluster_args(api.FROM_COMM) == (None, None, -1)
    flat, off, ncl = api._cluster_args([np.array([1, 3]), np.array([2])])
    assert ncl == 2 and flat.tolist() == [1, 3, 2] and off.tolist() == [0, 2, 3]
    assert api._cluster_args(None)[2] == 0 and api._cluster_args([])[2] == 0
