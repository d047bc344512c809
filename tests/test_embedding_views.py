"""CPU tests of the embedding views (cge_embedding_view: fp64 / fp32 / fp16 / bf16, host or device, either layout, with a leading
dimension): the entry points are declared and exported, the boundary check refuses what it must without a context or a GPU, and
`api.embedding_view` describes numpy arrays and torch tensors where they lie -- no copy -- or packs them once.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _lib():
    from cge.jl_amd import api

    L = api.load_library()
    L.cge_embedding_view_check.restype = C.c_int
    L.cge_embedding_view_check.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]
    return L


def _view(data, d, ld=0, dtype=0, on_device=0, row_major=1):
    from cge.jl_amd import api

    v = api.EmbeddingView()
    v.data, v.d, v.ld, v.dtype, v.on_device, v.row_major = data, d, ld, dtype, on_device, row_major
    return v


def _check(v, n):
    err = C.create_string_buffer(256)
    rc = _lib().cge_embedding_view_check(C.byref(v) if v is not None else None, n, err, 256)
    return rc, err.value.decode()


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    thdr = open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    assert re.search(r"int cge_embedding_view_check\(const cge_embedding_view \*v, int64_t n, char \*err, int64_t err_len\);", hdr)
    assert re.search(r"int cge_set_embedding_view\(cge_ctx \*ctx, const cge_embedding_view \*v, int64_t n\);", hdr)
    assert re.search(r"int cge_score_views\(cge_ctx \*ctx, const cge_score_args \*args, const cge_embedding_view \*views, int64_t K,", hdr)
    assert "} cge_embedding_view;" in hdr
    for name, code in (("F64", 0), ("F32", 1), ("F16", 2), ("BF16", 3)):
        assert re.search(rf"#define CGE_DTYPE_{name} {code}\b", hdr)
    assert "#define CGE_ABI_VERSION 1" in hdr  # additions only: the ABI version stays
    assert "int cge_resident_embedding_test(void *ctx, double *out, int64_t capacity_doubles, int64_t *rows, int64_t *d, int32_t *ids_out);" in thdr
    L = _lib()
    for sym in ("cge_embedding_view_check", "cge_set_embedding_view", "cge_score_views", "cge_resident_embedding_test"):
        assert hasattr(L, sym), sym
    assert L.cge_abi_version() == 1


def test_null_context_or_null_views_fail_at_the_boundary():
    from cge.jl_amd import api

    L = _lib()
    buf = np.zeros(8)
    v = _view(buf.ctypes.data, 2)
    a = api.ScoreArgs()
    out = np.zeros(7)
    olen = (C.c_int * 1)(5)
    assert L.cge_set_embedding_view(None, C.byref(v), C.c_int64(4)) == -7
    assert L.cge_score_views(None, C.byref(a), C.byref(v), C.c_int64(1), out.ctypes.data_as(C.c_void_p), olen, None) == -7
    assert L.cge_score_views(None, C.byref(a), None, C.c_int64(1), out.ctypes.data_as(C.c_void_p), olen, None) == -7
    rows, d = C.c_int64(), C.c_int64()
    assert L.cge_resident_embedding_test(None, None, C.c_int64(0), C.byref(rows), C.byref(d), None) == -7


def test_view_check_refuses_malformed_views():
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    n, d = 8, 4
    assert _check(None, n)[0] == -7
    assert _check(_view(None, d, dtype=1), n)[0] == -7  # NULL data
    assert _check(_view(p, 0, dtype=1), n)[0] == -7  # d = 0
    assert _check(_view(p, d, dtype=1), 0)[0] == -7  # n = 0
    assert _check(_view(p, d, dtype=4), n)[0] == -7  # unknown dtype
    assert _check(_view(p, d, dtype=-1), n)[0] == -7
    assert _check(_view(p, d, ld=d - 1, dtype=1, row_major=1), n)[0] == -7  # row-major: ld below d
    assert _check(_view(p, d, ld=n - 1, dtype=1, row_major=0), n)[0] == -7  # column-major: ld below n
    rc, msg = _check(_view(p + 1, d, dtype=1), n)  # an fp32 pointer at an odd byte address
    assert rc == -7 and "aligned" in msg
    assert _check(_view(p + 2, d, dtype=1), n)[0] == -7
    assert _check(_view(p + 1, d, dtype=3), n)[0] == -7
    assert _check(_view(p + 4, d, dtype=0), n)[0] == -7  # fp64 on a 4-byte boundary
    # every refusal comes with a message; err may be NULL
    assert all(_check(v, n)[1] for v in (_view(None, d), _view(p, 0), _view(p, d, dtype=4), _view(p, d, ld=d - 1)))
    assert _lib().cge_embedding_view_check(C.byref(_view(p, 0)), n, None, 0) == -7


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
@pytest.mark.parametrize("row_major", [0, 1])
@pytest.mark.parametrize("on_device", [0, 1])
def test_view_check_accepts_well_formed_views(dtype, row_major, on_device):
    buf = np.zeros(256)
    p = buf.ctypes.data
    n, d = 8, 4
    packed = d if row_major else n
    for ld in (0, packed, packed + 1, packed + 37):
        rc, msg = _check(_view(p, d, ld=ld, dtype=dtype, on_device=on_device, row_major=row_major), n)
        assert rc == 0 and msg == "", (ld, msg)
    es = (8, 4, 2, 2)[dtype]
    assert _check(_view(p + es, d, dtype=dtype, row_major=row_major), n)[0] == 0  # aligned to the element, no more


# ---- api.embedding_view ------------------------------------------------------------------------------------------------------
def _fields(v):
    return v.dtype, v.row_major, v.ld, v.d, v.on_device


def test_view_of_numpy_arrays_in_place():
    from cge.jl_amd import api

    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 24)).astype(np.float32)  # C order
    v, keep = api.embedding_view(a)
    assert _fields(v) == (api.DTYPE_F32, 1, 24, 24, 0) and v.data == a.ctypes.data and keep.shape == (40, 24)
    f = np.asfortranarray(rng.standard_normal((40, 24)))  # F order
    v, keep = api.embedding_view(f)
    assert _fields(v) == (api.DTYPE_F64, 0, 40, 24, 0) and v.data == f.ctypes.data
    h = rng.standard_normal((40, 24)).astype(np.float16)
    s = h[:, 3:19]  # a column slice of a C-order array: rows of 16 at a pitch of 24
    v, keep = api.embedding_view(s)
    assert _fields(v) == (api.DTYPE_F16, 1, 24, 16, 0) and v.data == h.ctypes.data + 3 * 2 and keep.shape == (40, 16)
    s = f[5:, :]  # a row slice of an F-order array: columns of 35 at a pitch of 40
    v, keep = api.embedding_view(s)
    assert _fields(v) == (api.DTYPE_F64, 0, 40, 24, 0) and v.data == f.ctypes.data + 5 * 8 and keep.shape == (35, 24)
    s = a[5:30, :]  # a row slice of a C-order array stays packed
    v, _ = api.embedding_view(s)
    assert _fields(v) == (api.DTYPE_F32, 1, 24, 24, 0) and v.data == a.ctypes.data + 5 * 24 * 4
    for v in (api.embedding_view(a)[0], api.embedding_view(f[5:, :])[0], api.embedding_view(h[:, 3:19])[0]):
        assert _check(v, 35)[0] == 0  # what it produces passes the boundary check


def test_view_of_a_memory_map_is_in_place(tmp_path):
    from cge.jl_amd import api

    path = os.path.join(tmp_path, "e.npy")
    np.save(path, np.arange(60, dtype=np.float32).reshape(12, 5))
    m = np.load(path, mmap_mode="r")
    v, keep = api.embedding_view(m)
    assert _fields(v) == (api.DTYPE_F32, 1, 5, 5, 0) and v.data == m.ctypes.data


def test_view_of_strided_or_other_arrays_is_one_packed_copy():
    from cge.jl_amd import api

    a = np.arange(40 * 24, dtype=np.float32).reshape(40, 24)
    s = a[::2, ::2]  # both axes strided
    v, keep = api.embedding_view(s)
    assert _fields(v) == (api.DTYPE_F32, 1, 12, 12, 0) and keep.dtype == np.float32 and np.array_equal(keep, s)
    assert v.data == keep.ctypes.data and keep.flags.c_contiguous
    v, keep = api.embedding_view(a[::-1, :])  # a negative stride
    assert _fields(v) == (api.DTYPE_F32, 1, 24, 24, 0) and np.array_equal(keep, a[::-1, :]) and keep.flags.c_contiguous
    i = np.arange(12, dtype=np.int32).reshape(4, 3)
    v, keep = api.embedding_view(i)
    assert _fields(v) == (api.DTYPE_F64, 1, 3, 3, 0) and keep.dtype == np.float64 and np.array_equal(keep, i)
    v, keep = api.embedding_view([[1, 2], [3, 4], [5, 6]])  # anything np.asarray takes
    assert _fields(v) == (api.DTYPE_F64, 1, 2, 2, 0)
    be = a.astype(">f4")  # not the machine's float32
    v, keep = api.embedding_view(be)
    assert v.dtype == api.DTYPE_F64 and np.array_equal(keep, a)
    with pytest.raises(TypeError):
        api.embedding_view(12345)
    with pytest.raises(ValueError):
        api.embedding_view(np.zeros(5))
    with pytest.raises(ValueError):
        api.embedding_view(np.zeros((0, 5)))


def test_view_of_single_row_and_single_column():
    from cge.jl_amd import api

    a = np.arange(7, dtype=np.float32).reshape(7, 1)
    v, _ = api.embedding_view(a)
    assert (v.d, v.data) == (1, a.ctypes.data) and _check(v, 7)[0] == 0
    b = np.arange(7, dtype=np.float64).reshape(1, 7)
    v, _ = api.embedding_view(b)
    assert (v.d, v.data) == (7, b.ctypes.data) and _check(v, 1)[0] == 0
    w = np.arange(21, dtype=np.float32).reshape(7, 3)[:, 1:2]  # one column of three: rows of 1 at a pitch of 3
    v, _ = api.embedding_view(w)
    assert _fields(v) == (api.DTYPE_F32, 1, 3, 1, 0) and v.data == w.ctypes.data


def test_view_of_torch_cpu_tensors_in_place():
    import torch
    from cge.jl_amd import api

    t = torch.arange(40 * 24, dtype=torch.float32).reshape(40, 24).to(torch.bfloat16)
    v, keep = api.embedding_view(t)
    assert _fields(v) == (api.DTYPE_BF16, 1, 24, 24, 0) and v.data == t.data_ptr()
    s = t[:, 1:17]  # 2-byte aligned and no more
    v, keep = api.embedding_view(s)
    assert _fields(v) == (api.DTYPE_BF16, 1, 24, 16, 0) and v.data == t.data_ptr() + 2 and _check(v, 40)[0] == 0
    tt = torch.zeros(24, 40, dtype=torch.float16).t()  # (40, 24) with strides (1, 40): column-major
    v, keep = api.embedding_view(tt)
    assert _fields(v) == (api.DTYPE_F16, 0, 40, 24, 0) and v.data == tt.data_ptr()
    g = torch.zeros(6, 4, dtype=torch.float64, requires_grad=True)
    v, keep = api.embedding_view(g)
    assert _fields(v) == (api.DTYPE_F64, 1, 4, 4, 0) and v.data == g.data_ptr()
    v, keep = api.embedding_view(t[::2, ::2])
    assert _fields(v) == (api.DTYPE_BF16, 1, 12, 12, 0) and keep.is_contiguous() and torch.equal(keep, t[::2, ::2])
    with pytest.raises(ValueError):
        api.embedding_view(torch.zeros(4, 4, dtype=torch.int32))


def test_compare_script_keeps_its_argument_split_and_reads_npy(tmp_path):
    import sys

    sys.path.insert(0, ROOT)
    try:
        import cge_compare
    finally:
        sys.path.pop(0)
    argv, files = cge_compare.split_embeddings(["-g", "g.txt", "-e", "a.npy", "-l", "400", "-e", "b.emb", "--seed", "1"])
    assert files == ["a.npy", "b.emb"]
    assert argv == ["-g", "g.txt", "-l", "400", "--seed", "1", "-e", "a.npy"]
    path = os.path.join(tmp_path, "e.npy")
    x = np.arange(30, dtype=np.float16).reshape(10, 3)
    np.save(path, x)
    m = cge_compare.read_any_embedding(path, 10)
    assert isinstance(m, np.memmap) and m.dtype == np.float16 and np.array_equal(m, x)
    with pytest.raises(AssertionError):
        cge_compare.read_any_embedding(path, 11)
