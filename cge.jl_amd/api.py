"""ctypes binding of libcge_hip.so + the host-side mirror of the reference's interface for the hot
path: ``landmarks`` (src/landmarks.jl:365-367), ``wGCL`` / ``wGCL_directed`` (src/divergence.jl:27-31,
:282-286) with the reference's positional arguments, and ``score`` = example/CGE_CLI.jl:10-24 on
device-resident inputs.

There is no CPU path here: if the library is missing or no GPU is visible every compute entry point
raises ``CGEError``.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

from .args import _SplitRule

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "csrc", "build", "libcge_hip.so")
_lib = None

CGE_OK = 0
_CODES = {-1: "AssertionError", -2: "ErrorException: Trying to split homogenous cluster",
          -3: "ErrorException: Unexpected empty cluster generated", -4: "HIP error / no GPU",
          -5: "collective hook failed", -6: "out of memory", -7: "bad argument"}


class CGEError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"{_CODES.get(code, 'error')} (code {code}){': ' + msg if msg else ''}")
        self.code = code


class AssertionErrorCGE(CGEError, AssertionError):
    """A reference ``@assert`` fired (src/divergence.jl:50,81,303,363; src/landmarks.jl:93,...)."""


class WgclArgs(C.Structure):
    _fields_ = [("edges_src", C.c_void_p), ("edges_dst", C.c_void_p), ("eweights", C.c_void_p), ("m", C.c_int64),
                ("comm", C.c_void_p), ("n_comm", C.c_int64), ("embed", C.c_void_p), ("embed_rows", C.c_int64),
                ("d", C.c_int64), ("distances", C.c_void_p), ("n_distances", C.c_int64), ("vweights", C.c_void_p),
                ("init_vweights", C.c_void_p), ("n_init", C.c_int64), ("v_to_l", C.c_void_p),
                ("n_v_to_l", C.c_int64), ("init_edges_src", C.c_void_p), ("init_edges_dst", C.c_void_p),
                ("m_init", C.c_int64), ("init_eweights", C.c_void_p), ("init_embed", C.c_void_p), ("split", C.c_int),
                ("seed", C.c_int64), ("auc_samples", C.c_int64), ("verbose", C.c_int), ("directed", C.c_int),
                ("pos_idx", C.c_void_p), ("neg_i", C.c_void_p), ("neg_j", C.c_void_p), ("pos_idx2", C.c_void_p),
                ("n_sample_sets", C.c_int64)]


class Trace(C.Structure):
    _fields_ = [("n_alpha", C.c_int64), ("iters", C.c_int64 * 64), ("div", C.c_double * 64),
                ("auc", C.c_double * 64)]

    def as_dict(self):
        k = self.n_alpha
        return {"n_alpha": k, "iters": list(self.iters[:k]), "div": list(self.div[:k]), "auc": list(self.auc[:k])}


class ScoreArgs(C.Structure):
    _fields_ = [("clusters_flat", C.c_void_p), ("clusters_off", C.c_void_p), ("n_clusters", C.c_int64),
                ("land", C.c_int64), ("forced", C.c_int64), ("method", C.c_int), ("directed", C.c_int),
                ("split", C.c_int), ("seed", C.c_int64), ("auc_samples", C.c_int64)]


class EcgArgs(C.Structure):
    """cge_ecg_args (include/cge_hip.h)."""
    _fields_ = [("members", C.c_int64), ("w_min", C.c_double), ("seed", C.c_int64), ("final_level", C.c_int64)]


class EmbeddingBatch(C.Structure):
    _fields_ = [("embeddings", C.c_void_p), ("K", C.c_int64), ("d", C.c_int64), ("on_device", C.c_int),
                ("row_major", C.c_int)]


class EmbeddingView(C.Structure):
    """cge_embedding_view (include/cge_hip.h): an (n, d) embedding where and as its owner holds it."""
    _fields_ = [("data", C.c_void_p), ("d", C.c_int64), ("ld", C.c_int64), ("dtype", C.c_int), ("on_device", C.c_int),
                ("row_major", C.c_int)]


class GraphView(C.Structure):
    """cge_graph_view (include/cge_hip.h): an edge list where and as its owner holds it."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("stride", C.c_int64), ("id_dtype", C.c_int), ("base", C.c_int),
                ("w", C.c_void_p), ("w_dtype", C.c_int), ("on_device", C.c_int)]


class VertexView(C.Structure):
    """cge_vertex_view (include/cge_hip.h): community ids and (optionally) vertex weights where their owner holds them."""
    _fields_ = [("comm", C.c_void_p), ("id_dtype", C.c_int), ("base", C.c_int), ("vweights", C.c_void_p), ("vw_dtype", C.c_int),
                ("on_device", C.c_int)]


class ResidentGraph(C.Structure):
    """cge_resident_graph (include/cge_hip_testing.h)."""
    _fields_ = [("n", C.c_int64), ("m", C.c_int64), ("n_comm_max", C.c_int64), ("n_comm16", C.c_int64), ("unit", C.c_int),
                ("have", C.c_int), ("src", C.c_void_p), ("dst", C.c_void_p), ("comm", C.c_void_p), ("w", C.c_void_p),
                ("vweight", C.c_void_p), ("comm16", C.c_void_p), ("cap_edges", C.c_int64), ("cap_vertices", C.c_int64),
                ("cap_comm16", C.c_int64)]


class VectBProblem(C.Structure):
    """cge_vect_b_problem (include/cge_hip_testing.h): one problem of the testing hook cge_vect_b_test."""
    _fields_ = [("GD", C.c_void_p), ("Ta", C.c_void_p), ("Tb", C.c_void_p), ("comm", C.c_void_p), ("N", C.c_int64),
                ("C", C.c_int64), ("vC", C.c_void_p), ("vectB", C.c_void_p), ("js_dev", C.c_void_p), ("js_fused", C.c_void_p)]


VECT_B_GUARD = 64  # CGE_VECT_B_GUARD


class FitProblem(C.Structure):
    """cge_fit_problem (include/cge_hip_testing.h): one problem of the testing hook cge_fit_test."""
    _fields_ = [("D", C.c_void_p), ("w", C.c_void_p), ("w2", C.c_void_p), ("T0", C.c_void_p), ("T0b", C.c_void_p),
                ("T", C.c_void_p), ("Tb", C.c_void_p), ("GD", C.c_void_p), ("N", C.c_int64), ("alpha", C.c_double),
                ("iters", C.c_int64), ("status", C.c_int32), ("pad", C.c_int32)]


class FusedChainProblem(C.Structure):
    """cge_fused_chain_problem (include/cge_hip_testing.h): one problem of the testing hook cge_fused_chain_test."""
    _fields_ = [("D", C.c_void_p), ("w", C.c_void_p), ("T0", C.c_void_p), ("comm", C.c_void_p), ("N", C.c_int64),
                ("C", C.c_int64), ("alpha", C.c_double), ("vC", C.c_void_p), ("want", C.c_int32), ("n_modes", C.c_int32),
                ("S", C.c_int64), ("aidx", C.c_void_p), ("afac", C.c_void_p), ("aden", C.c_void_p), ("dpos", C.c_void_p),
                ("dneg", C.c_void_p), ("wts", C.c_void_p), ("T", C.c_void_p), ("order", C.c_void_p), ("fc", C.c_void_p),
                ("ns", C.c_void_p), ("base", C.c_void_p), ("partials", C.c_void_p), ("partials_cap", C.c_int64),
                ("bt_total", C.c_int64), ("vectB", C.c_void_p), ("js_fused", C.c_void_p), ("part", C.c_void_p),
                ("apw", C.c_void_p), ("iters", C.c_int64), ("status", C.c_int32), ("pad", C.c_int32)]


class LandmarkGraphIO(C.Structure):
    """cge_landmark_graph_io (include/cge_hip_testing.h): the arguments of the testing hook cge_landmark_graph_test."""
    _fields_ = [("v2l", C.c_void_p), ("N", C.c_int64), ("directed", C.c_int32), ("wedge_form", C.c_int32), ("part", C.c_int64),
                ("nparts", C.c_int64), ("world", C.c_int64), ("lemb", C.c_void_p), ("lweight", C.c_void_p), ("dii", C.c_void_p),
                ("lcomm", C.c_void_p), ("wedges", C.c_void_p), ("positive", C.c_void_p), ("deg_out", C.c_void_p),
                ("deg_in", C.c_void_p), ("star", C.c_void_p), ("deg_block", C.c_void_p), ("u_deg_out", C.c_void_p),
                ("u_deg_in", C.c_void_p), ("u_star", C.c_void_p), ("n_chunks", C.c_int64), ("ntile", C.c_int64),
                ("form_ran", C.c_int32), ("rshift", C.c_int32), ("colbits", C.c_int32), ("pad", C.c_int32)]


class SweepSetupIO(C.Structure):
    """cge_sweep_setup_io (include/cge_hip_testing.h): the arguments of the testing hook cge_sweep_setup_test."""
    _fields_ = [("emb", C.c_void_p), ("dist", C.c_void_p), ("vw", C.c_void_p), ("comm", C.c_void_p), ("N", C.c_int64),
                ("d", C.c_int64), ("C", C.c_int64), ("directed", C.c_int32), ("landmarks", C.c_int32),
                ("force_relabel", C.c_int32), ("log_form", C.c_int32), ("alpha", C.c_double), ("src", C.c_void_p),
                ("dst", C.c_void_p), ("w", C.c_void_p), ("m", C.c_int64),
                ("deg_out", C.c_void_p), ("deg_in", C.c_void_p), ("star", C.c_void_p),
                ("order", C.c_void_p), ("old2new", C.c_void_p), ("comm_rl", C.c_void_p), ("cm_off", C.c_void_p),
                ("cm_mem", C.c_void_p), ("cm_pos", C.c_void_p), ("emb_rl", C.c_void_p), ("vec_rl", C.c_void_p),
                ("D_raw", C.c_void_p), ("lo_hi", C.c_void_p), ("D", C.c_void_p),
                ("Lh", C.c_void_p), ("Ll", C.c_void_p), ("log_cap", C.c_int64), ("log_count", C.c_int64), ("GD", C.c_void_p),
                ("T1", C.c_void_p), ("T2", C.c_void_p), ("TT", C.c_void_p), ("Tld", C.c_int64), ("relabel", C.c_int32),
                ("log_form_ran", C.c_int32)]


class LocalScoreIO(C.Structure):
    """cge_local_score_io (include/cge_hip_testing.h): the arguments of the testing hook cge_local_score_test."""
    _fields_ = [("S", C.c_int64), ("seed", C.c_int64), ("stream_id", C.c_int64), ("directed", C.c_int32),
                ("draw_route", C.c_int32), ("form", C.c_int32), ("sharded", C.c_int32),
                ("pos", C.c_void_p), ("neg_i", C.c_void_p), ("neg_j", C.c_void_p), ("attempt", C.c_void_p), ("rounds", C.c_int64),
                ("pos_in", C.c_void_p), ("pos2_in", C.c_void_p), ("neg_i_in", C.c_void_p), ("neg_j_in", C.c_void_p),
                ("pi", C.c_void_p), ("pj", C.c_void_p), ("ni", C.c_void_p), ("nj", C.c_void_p), ("wts", C.c_void_p),
                ("pi_in", C.c_void_p), ("pj_in", C.c_void_p), ("ni_in", C.c_void_p), ("nj_in", C.c_void_p),
                ("wts_in", C.c_void_p), ("hi", C.c_double), ("dpos", C.c_void_p), ("dneg", C.c_void_p),
                ("dpos_in", C.c_void_p), ("dneg_in", C.c_void_p), ("N", C.c_int64), ("alpha", C.c_double),
                ("Ta", C.c_void_p), ("Tb", C.c_void_p), ("vw", C.c_void_p), ("lweight", C.c_void_p), ("GD", C.c_void_p),
                ("v2l", C.c_void_p), ("old2new", C.c_void_p), ("part", C.c_void_p), ("out2", C.c_void_p),
                ("D", C.c_void_p), ("w", C.c_void_p), ("T0", C.c_void_p), ("eps", C.c_double), ("delta", C.c_double),
                ("T", C.c_void_p), ("afac", C.c_void_p), ("aden", C.c_void_p), ("aidx", C.c_void_p), ("iters", C.c_int64),
                ("status", C.c_int32), ("pad2", C.c_int32)]


DTYPE_F64, DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2, 3
_NP_DTYPES = {np.dtype(np.float64): DTYPE_F64, np.dtype(np.float32): DTYPE_F32, np.dtype(np.float16): DTYPE_F16}

ID_I64, ID_I32 = 0, 1


class _FromComm:
    """`clusters=FROM_COMM`: the clusters parseargs builds from the communities (src/auxilary.jl:199-208), derived by the library
    from the resident community vector (n_clusters = -1 of the C-ABI)."""

    def __repr__(self):
        return "FROM_COMM"


FROM_COMM = _FromComm()

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)


class Collectives(C.Structure):
    _fields_ = [("allreduce_f64", ALLREDUCE_FN), ("user", C.c_void_p), ("rank", C.c_int), ("world", C.c_int)]


GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)  # (user, buf, words per rank): all-gather / reduce-scatter


class CollectivesExt(C.Structure):
    _fields_ = [("allgather", GATHER_FN), ("reduce_scatter_f64", GATHER_FN)]


# Live contexts are closed from an `atexit` hook: it runs inside Py_Finalize, i.e. BEFORE the C-level exit handlers
# of the HIP runtime and of a profiler's tool library, so no stream or event of this library is left for the runtime to
# destroy after a profiler has finalised its HSA hooks.  DEFENCE IN DEPTH ONLY: it is NOT an established fix for the
# exit-time SIGSEGV under rocprofv3 recorded in round 1 -- a probe that left a context alive with this hook disabled exited
# cleanly, so the cause of that fault is still unproven (the cooperative launches that build used
# are gone; the fault has not reappeared in any record since).
_live = weakref.WeakSet()
_atexit_registered = False


def _close_live_contexts():
    for ctx in list(_live):
        try:
            ctx.close()
        except Exception:
            pass


def library_path():
    return _LIB_PATH


def load_library():
    """Load libcge_hip.so; raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise CGEError(-4, f"{_LIB_PATH} not found: build it with `make -C cge.jl_amd/csrc` "
                               f"(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(_LIB_PATH)
        L.cge_last_error.restype = C.c_char_p
        L.cge_last_error.argtypes = [C.c_void_p]
        L.cge_idx.restype = C.c_int64
        L.cge_idx.argtypes = [C.c_int64] * 3
        L.cge_destroy.argtypes = [C.c_void_p]
        L.cge_destroy.restype = None
        _lib = L
    return _lib


def read_table(path, column_major=True, n_threads=0):
    """Numeric text table -> float64 array (rows, cols) through the library's parallel reader
    (include/cge_hip.h: cge_text_table_*; replaces `readdlm`, src/auxilary.jl:80-168).  Needs no GPU.
    Returns (array, header_skipped)."""
    L = load_library()
    L.cge_text_table_close.argtypes = [C.c_void_p]
    L.cge_text_table_close.restype = None
    rows, cols, hdr, h = C.c_int64(), C.c_int64(), C.c_int(), C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.cge_text_table_open(os.fsencode(path), C.c_int(n_threads), C.byref(rows), C.byref(cols), C.byref(hdr),
                               C.byref(h), err, C.c_int64(512))
    if rc != 0:
        raise CGEError(rc, err.value.decode() or f"cannot read {path}")
    try:
        out = np.empty((rows.value, cols.value), dtype=np.float64, order="F" if column_major else "C")
        rc = L.cge_text_table_parse(h, out.ctypes.data_as(C.c_void_p), C.c_int(1 if column_major else 0), err,
                                    C.c_int64(512))
        if rc != 0:
            raise CGEError(rc, err.value.decode() or f"cannot parse {path}")
    finally:
        L.cge_text_table_close(h)
    return out, bool(hdr.value)


def _method_code(method):
    if isinstance(method, _SplitRule):
        return method.code
    if isinstance(method, str):
        return {"rss": 0, "rss2": 1, "size": 2, "diameter": 3}[method]
    return int(method)


def wedge_geometry_test(N, weighted, n_chunks):
    """Host-only hook (include/cge_hip_testing.h: cge_wedge_geometry_test): the geometry of the tiled form of the landmark-pair
    matrix.  None where the form declines, else a dict rshift, colbits, ntile, lds_pass1, lds_pass2."""
    L = load_library()
    ap, rs, cb = C.c_int(), C.c_int(), C.c_int()
    nt, l1, l2 = C.c_int64(), C.c_int64(), C.c_int64()
    rc = L.cge_wedge_geometry_test(C.c_int64(N), C.c_int(int(bool(weighted))), C.c_int64(n_chunks), C.byref(ap), C.byref(rs),
                                   C.byref(cb), C.byref(nt), C.byref(l1), C.byref(l2))
    if rc:
        raise CGEError(rc, "cge_wedge_geometry_test")
    if not ap.value:
        return None
    return {"rshift": rs.value, "colbits": cb.value, "ntile": nt.value, "lds_pass1": l1.value, "lds_pass2": l2.value}


def fit_dir_geometry_test(N, cus):
    """Host-only hook (include/cge_hip_testing.h: cge_fit_dir_geometry_test): the one geometry of the persistent fits, undirected
    and directed, for N vertices on `cus` CUs.  None where the form declines, else (G, NW, NSB)."""
    L = load_library()
    ap, G, NW, NSB = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = L.cge_fit_dir_geometry_test(C.c_int64(N), C.c_int(cus), C.byref(ap), C.byref(G), C.byref(NW), C.byref(NSB))
    if rc:
        raise CGEError(rc, "cge_fit_dir_geometry_test")
    return (G.value, NW.value, NSB.value) if ap.value else None


def fit_slots_test(N, directed):
    """Host-only hook (cge_fit_slots_test): the hand-off slots of one persistent-fit problem of N vertices with Tld = 64 Nt, in
    doubles from the start of its region: a dict sync, ring, fq, P (offsets) and doubles (the region's length)."""
    L = load_library()
    out = (C.c_int64 * 5)()
    rc = L.cge_fit_slots_test(C.c_int64(N), C.c_int(int(bool(directed))), out)
    if rc:
        raise CGEError(rc, "cge_fit_slots_test")
    return dict(zip(("sync", "ring", "fq", "P", "doubles"), (int(v) for v in out)))


def batch_pack_dir_test(N, cus):
    """Host-only hook (cge_batch_pack_dir_test): the launch groups of a directed batch whose members have N[k] landmarks on
    `cus` CUs.  Returns (number of groups, group_of) with group_of[k] = -1 for a member that is scored on its own."""
    L = load_library()
    N = np.ascontiguousarray(N, dtype=np.int64)
    out = np.full(len(N), -2, np.int32)
    L.cge_batch_pack_dir_test.restype = C.c_int
    L.cge_batch_pack_dir_test.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    n = L.cge_batch_pack_dir_test(N.ctypes.data, len(N), int(cus), out.ctypes.data)
    if n < 0:
        raise CGEError(n, "cge_batch_pack_dir_test")
    return n, out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _host_array(x):  # a numpy array of a numpy array, a sequence or a torch tensor (any device)
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _colmajor(a):  # (rows, cols) array -> flat buffer in Julia (column-major) order
    a = np.asfortranarray(np.asarray(a, dtype=np.float64))
    return a, a.ravel(order="K")


def _view_layout(n, d, s0, s1):
    """(row_major, ld) of an (n, d) matrix with element strides (s0, s1) that a view can describe in place -- unit stride along
    one axis, the other at least the packed pitch -- or None (both axes strided, a negative or a zero stride)."""
    if (d == 1 or s1 == 1) and (n == 1 or s0 >= d):
        return 1, (s0 if n > 1 else d)
    if (n == 1 or s0 == 1) and (d == 1 or s1 >= n):
        return 0, (s1 if d > 1 else n)
    return None


def embedding_view(x):
    """(EmbeddingView, owner) for an (n, d) embedding, described where it lies; needs no GPU.  `owner` is the array or tensor the
    view points into (n = owner.shape[0]); keep it alive while the view is in use.

    numpy arrays of float64 / float32 / float16 and torch tensors (any device) of float64 / float32 / float16 / bfloat16 that
    are C- or F-contiguous, or a 2-D slice of such a matrix (unit stride along one axis: `X[:, :64]`, `X[5:, :]`), are taken in
    place: no copy, the leading dimension comes from the strides.  Any other striding costs one packed copy in the same dtype;
    other numpy dtypes (integers, ...) become float64, as `set_embedding` makes them.  A plain int is not accepted (raw device
    pointers: `Context.set_embedding_device`)."""
    if isinstance(x, (int, np.integer)):
        raise TypeError("embedding_view: a raw pointer is not a view (Context.set_embedding_device takes device pointers)")
    torch = sys.modules.get("torch")
    v = EmbeddingView()
    if torch is not None and isinstance(x, torch.Tensor):
        codes = {torch.float64: DTYPE_F64, torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}
        t = x.detach()
        if t.dtype not in codes:
            raise ValueError(f"embedding_view: tensor dtype {t.dtype} (float64, float32, float16 or bfloat16)")
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("embedding_view: an embedding is a non-empty (n, d) matrix")
        lay = _view_layout(t.shape[0], t.shape[1], *t.stride())
        if lay is None:
            t = t.contiguous()
            lay = 1, t.shape[1]
        v.data, v.d, v.dtype, v.on_device = t.data_ptr(), t.shape[1], codes[t.dtype], int(t.is_cuda)
        v.row_major, v.ld = lay
        return v, t
    a = np.asarray(x)
    if a.dtype not in _NP_DTYPES:
        a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("embedding_view: an embedding is a non-empty (n, d) matrix")
    sz = a.dtype.itemsize
    lay = None if a.strides[0] % sz or a.strides[1] % sz else _view_layout(a.shape[0], a.shape[1], a.strides[0] // sz, a.strides[1] // sz)
    if lay is None:
        a = np.ascontiguousarray(a)
        lay = 1, a.shape[1]
    v.data, v.d, v.dtype, v.on_device = a.ctypes.data, a.shape[1], _NP_DTYPES[a.dtype], 0
    v.row_major, v.ld = lay
    return v, a


def _as_described(x, int_ids, what):
    """(owner, pointer, itemsize, element strides or None, dtype code, on_device) of a numpy array or torch tensor taken as it is:
    ids are int32 / int64 (anything else becomes int64), reals float64 / float32 (anything else becomes float64)."""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(x, torch.Tensor):
        t = x.detach()
        codes = {torch.int64: ID_I64, torch.int32: ID_I32} if int_ids else {torch.float64: DTYPE_F64, torch.float32: DTYPE_F32}
        if t.dtype not in codes:
            t = t.to(torch.int64 if int_ids else torch.float64)
        return t, t.data_ptr(), t.element_size(), tuple(t.stride()), codes[t.dtype], int(t.is_cuda)
    if isinstance(x, (int, np.integer)):
        raise TypeError(f"{what}: a raw pointer is not a view")
    a = np.asarray(x)
    codes = ({np.dtype(np.int64): ID_I64, np.dtype(np.int32): ID_I32} if int_ids else
             {np.dtype(np.float64): DTYPE_F64, np.dtype(np.float32): DTYPE_F32})
    if a.dtype not in codes:
        a = np.asarray(a, dtype=np.int64 if int_ids else np.float64)
    sz = a.dtype.itemsize
    strides = None if any(b % sz for b in a.strides) else tuple(b // sz for b in a.strides)
    return a, a.ctypes.data, sz, strides, codes[a.dtype], 0


def _packed(owner):
    """One packed (C-order) copy in the same dtype, where the owner lives."""
    return owner.contiguous() if hasattr(owner, "contiguous") else np.ascontiguousarray(owner)


def _flat_vector(x, int_ids, what):
    """A 1-D (or (n, 1) / (1, n)) vector described in place when it has unit stride, packed once otherwise."""
    owner, ptr, sz, strides, code, dev = _as_described(x, int_ids, what)
    if owner.ndim == 2 and 1 in tuple(owner.shape):
        owner = owner.reshape(-1)
        owner, ptr, sz, strides, code, dev = _as_described(owner, int_ids, what)
    if owner.ndim != 1 or owner.shape[0] < 1:
        raise ValueError(f"{what}: a non-empty vector is expected")
    if owner.shape[0] > 1 and (strides is None or strides[0] != 1):
        owner = _packed(owner)
        owner, ptr, sz, strides, code, dev = _as_described(owner, int_ids, what)
    return owner, ptr, code, dev


def graph_view(edge_index, weights=None, base=-1):
    """(GraphView, owners, m) for an edge list described where it lies; needs no GPU.  Keep `owners` alive while the view is in use.

    `edge_index`: a numpy array or a torch tensor (any device) of shape (2, m) -- PyG's edge_index -- or (m, 2) -- the reference's
    `edges` --, int32 or int64; a (2, 2) array is taken as (2, m).  C- and F-ordered arrays, slices (`ei[:, 1:]`) and regular steps
    are taken in place: the two endpoint columns and their common stride come from the array's strides.  One packed copy in the
    same dtype is made only when no stride form fits (a negative or zero step); other dtypes become int64.  `weights`: m edge
    weights, float64 / float32 (others become float64), in the same place (host / GPU) as the ids; None = an unweighted list.
    `base`: 0 or 1, or -1 to decide it as parseargs does (the minimum id must be 0 or 1)."""
    owner, ptr, sz, strides, code, dev = _as_described(edge_index, True, "graph_view")
    if owner.ndim != 2 or 2 not in tuple(owner.shape) or 0 in tuple(owner.shape):
        raise ValueError("graph_view: an edge list is a non-empty (2, m) or (m, 2) array")
    rows = owner.shape[0] == 2  # (2, m): the endpoints are the two rows
    m = int(owner.shape[1] if rows else owner.shape[0])

    def form(strides):
        if strides is None:
            return None
        col, step = (strides[0], strides[1]) if rows else (strides[1], strides[0])  # endpoint offset, step from edge to edge
        if m == 1:
            step = 1
        return (col, step) if step >= 1 and col != 0 else None

    f = form(strides)
    if f is None:
        owner = _packed(owner)
        owner, ptr, sz, strides, code, dev = _as_described(owner, True, "graph_view")
        f = form(strides)
    g = GraphView()
    g.src, g.dst, g.stride, g.id_dtype, g.base, g.on_device = ptr, ptr + f[0] * sz, f[1], code, int(base), dev
    owners = [owner]
    if weights is not None:
        w, wptr, wcode, wdev = _flat_vector(weights, False, "graph_view: weights")
        if w.shape[0] != m:
            raise ValueError(f"graph_view: {w.shape[0]} weights for {m} edges")
        if wdev != dev:
            raise ValueError("graph_view: the ids and the weights must both be on the host or both on the GPU")
        g.w, g.w_dtype = wptr, wcode
        owners.append(w)
    return g, owners, m


def vertex_view(comm, vweights=None, base=-1):
    """(VertexView, owners, n) for community ids (n, or (n, 1); int32 / int64; None leaves the resident ones) and vertex weights
    (float64 / float32; None = derive them from the resident edge list, src/auxilary.jl:104-110), described where they lie."""
    v = VertexView()
    v.base = int(base)
    owners, n, dev = [], None, None
    if comm is not None:
        c, ptr, code, dev = _flat_vector(comm, True, "vertex_view: comm")
        v.comm, v.id_dtype, n = ptr, code, int(c.shape[0])
        owners.append(c)
    if vweights is not None:
        w, wptr, wcode, wdev = _flat_vector(vweights, False, "vertex_view: vweights")
        if n is not None and (w.shape[0] != n or wdev != dev):
            raise ValueError("vertex_view: comm and vweights must have one length and one place (host or GPU)")
        v.vweights, v.vw_dtype, n, dev = wptr, wcode, int(w.shape[0]), wdev
        owners.append(w)
    v.on_device = int(dev or 0)
    return v, owners, n


def clusters_of(comm):
    """parseargs' clusters (src/auxilary.jl:199-208) of a community vector, in pure Python: one list of 1-based vertex ids per
    community that occurs, ascending inside a cluster, clusters by ascending community id.  What FROM_COMM derives."""
    groups = {}
    for i, q in enumerate(np.asarray(comm).ravel().tolist()):
        groups.setdefault(q, []).append(i + 1)
    return [np.asarray(groups[q], dtype=np.int64) for q in sorted(groups)]


def _cluster_args(clusters):
    """(flat, off, n_clusters) as the C-ABI takes clusters; FROM_COMM: n_clusters = -1, no arrays."""
    if clusters is FROM_COMM:
        return None, None, -1
    flat, off = _flatten_clusters(clusters if clusters is not None and len(clusters) else [])
    return flat, off, len(off) - 1


def _edge_cols(edges):
    e = np.asarray(edges, dtype=np.int64)
    if e.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])


class FlatClusters:
    """`clusters::Vector{Vector{Int}}` (src/auxilary.jl:199-208) in the form the C-ABI takes: member ids back to back + offsets.
    Build it once with `flatten_clusters` and hand it to `Context.score` / `landmarks_run` instead of the list of lists when
    the same clusters are scored repeatedly (flattening a million ids is ~1 ms of numpy per call)."""

    def __init__(self, flat, off):
        self.flat, self.off = flat, off

    def __len__(self):
        return len(self.off) - 1


def flatten_clusters(clusters):
    return FlatClusters(*_flatten_clusters_raw(clusters))


_flat_cache = {}  # id(list) -> (fingerprint, FlatClusters): the last few lists of clusters seen, by identity


def _flatten_clusters(clusters):
    """Flat form of a list of clusters.  A list object that was flattened before is recognised by identity (the list and every
    member array: ids and lengths) and its flat form reused -- callers that score the same clusters again and again (bench.py,
    a sweep over embeddings) then pay the ~1 ms of concatenation once.  Contract: do not change a cluster's members IN PLACE
    between calls; build a new list (or a FlatClusters) instead."""
    if isinstance(clusters, FlatClusters):
        return clusters.flat, clusters.off
    if isinstance(clusters, list) and len(clusters) > 16:
        fp = (len(clusters), tuple((id(c), len(c)) for c in clusters))
        hit = _flat_cache.get(id(clusters))
        if hit is not None and hit[0] == fp:
            return hit[1].flat, hit[1].off
        fc = flatten_clusters(clusters)
        if len(_flat_cache) >= 4:
            _flat_cache.pop(next(iter(_flat_cache)))
        _flat_cache[id(clusters)] = (fp, fc, clusters)  # (the list is kept alive: its id cannot be reused while the entry lives)
        return fc.flat, fc.off
    return _flatten_clusters_raw(clusters)


def _flatten_clusters_raw(clusters):
    off = np.zeros(len(clusters) + 1, dtype=np.int64)
    for k, c in enumerate(clusters):
        off[k + 1] = off[k] + len(c)
    flat = np.concatenate([np.asarray(c, dtype=np.int64) for c in clusters]) if len(clusters) else np.zeros(0, np.int64)
    return np.ascontiguousarray(flat), off


class Context:
    """One GPU, one stream.  Not re-entrant (one host thread drives it)."""

    def __init__(self, device: int = 0, stream=None):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.cge_create(C.byref(h), C.c_int(device), C.c_void_p(stream) if stream else None)
        if rc:
            raise CGEError(rc, "cge_create failed (no MI355X visible?)")
        self.h = h
        self.device = device
        self.stream = int(stream) if stream else None
        self._keep = []  # objects the C side holds pointers to (collective hook)
        self.n = self.m = self.d = 0
        global _atexit_registered
        _live.add(self)
        if not _atexit_registered and not os.environ.get("CGE_NO_ATEXIT_CLOSE"):
            atexit.register(_close_live_contexts)
            _atexit_registered = True

    def close(self):
        if getattr(self, "h", None):
            self.L.cge_destroy(self.h)
            self.h = None
        _live.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            msg = self.L.cge_last_error(self.h).decode(errors="replace")
            raise (AssertionErrorCGE if rc == -1 else CGEError)(rc, msg)

    # ---- resident inputs ------------------------------------------------------------------------
    def set_host_threads(self, n):
        self._check(self.L.cge_set_host_threads(self.h, C.c_int(n)))

    def set_graph(self, edges, eweights, n):
        s, t = _edge_cols(edges)
        w = _f64(eweights)
        self._check(self.L.cge_set_graph(self.h, _p(s), _p(t), _p(w), C.c_int64(len(s)), C.c_int64(n)))
        self.m, self.n = len(s), n

    def set_embedding(self, embedding):
        e, ef = _colmajor(embedding)
        self._check(self.L.cge_set_embedding(self.h, _p(ef), C.c_int64(e.shape[0]), C.c_int64(e.shape[1])))
        self.d = e.shape[1]

    def set_embedding_device(self, dev_ptr: int, n: int, d: int, row_major: bool = True):
        """An (n, d) float64 embedding that already lives in this GPU's memory (e.g. `tensor.data_ptr()`)."""
        self._check(self.L.cge_set_embedding_device(self.h, C.c_void_p(dev_ptr), C.c_int64(n), C.c_int64(d),
                                                    C.c_int(1 if row_major else 0)))
        self.d = d

    def _view(self, x):
        """`embedding_view(x)`, ready for a call on this context: a CUDA tensor must live on the context's GPU, and what its
        current torch stream has enqueued is finished first (unless that stream is the context's own)."""
        v, owner = embedding_view(x)
        if v.on_device:
            self._sync_with(owner)
        return v, owner

    def set_embedding_view(self, x):
        """The (n, d) embedding `x` -- a numpy array or a torch tensor, on the host or on this GPU, float64 / float32 / float16
        (/ bfloat16), C- or F-ordered or a slice -- made resident as it is (cge_set_embedding_view): it travels in its own type and
        is widened to float64 on the device, which is exact.  Same results as `set_embedding(x.astype(float64))`."""
        v, owner = self._view(x)
        self._check(self.L.cge_set_embedding_view(self.h, C.byref(v), C.c_int64(owner.shape[0])))
        self.d = int(v.d)

    def resident_embedding(self):
        """Testing hook (include/cge_hip_testing.h): (rows held by this rank as an (r, d) float64 array, their 0-based ids)."""
        r, d = C.c_int64(), C.c_int64()
        self.L.cge_resident_embedding_test(self.h, None, C.c_int64(0), C.byref(r), C.byref(d), None)  # (the sizes)
        out, ids = np.empty((r.value, d.value)), np.empty(r.value, dtype=np.int32)
        self._check(self.L.cge_resident_embedding_test(self.h, _p(out), C.c_int64(out.size), C.byref(r), C.byref(d), _p(ids)))
        return out, ids

    def _sync_with(self, owner):
        """A CUDA tensor handed to this context: it must live on the context's GPU, and what its current torch stream has
        enqueued is finished first (unless that stream is the context's own)."""
        import torch

        if owner.device.index != self.device:
            raise ValueError(f"tensor on {owner.device}, the context is on GPU {self.device}")
        st = torch.cuda.current_stream(owner.device)
        if self.stream is None or st.cuda_stream != self.stream:
            st.synchronize()

    def set_graph_view(self, edge_index, weights=None, n=0, base=-1):
        """The edge list as held -- `api.graph_view(edge_index, weights, base)`: a (2, m) or (m, 2) int32 / int64 numpy array or
        torch tensor, 0- or 1-based, on the host or on this GPU -- made the resident graph (cge_set_graph_view): the same resident
        state as `set_graph` of the same edges.  n = 0: the vertex count is the maximum id.  Returns n."""
        g, owners, m = graph_view(edge_index, weights, base)
        if g.on_device:
            for o in owners:
                self._sync_with(o)
        n_out = C.c_int64()
        self._check(self.L.cge_set_graph_view(self.h, C.byref(g), C.c_int64(m), C.c_int64(int(n)), C.byref(n_out)))
        self.m, self.n = m, n_out.value
        del owners
        return self.n

    def set_vertex_view(self, comm, vweights=None, base=-1):
        """Community ids (and vertex weights) as held (`api.vertex_view`); vweights=None derives them from the resident edge
        list in the reference's order of addition (src/auxilary.jl:104-110)."""
        v, owners, n = vertex_view(comm, vweights, base)
        if n is None:
            n = self.n
        if v.on_device:
            for o in owners:
                self._sync_with(o)
        self._check(self.L.cge_set_vertex_view(self.h, C.byref(v), C.c_int64(n)))
        del owners

    def vertex_weights(self):
        """The resident vweight (n,), e.g. the derived one, for `wGCL`'s vweights argument (cge_vertex_weights)."""
        out = np.empty(self.n)
        self._check(self.L.cge_vertex_weights(self.h, _p(out), C.c_int64(self.n)))
        return out

    def resident_graph(self):
        """Testing hook (include/cge_hip_testing.h: cge_resident_graph_test): what the context holds, copied from the device:
        dict(n, m, unit, n_comm_max, src, dst (int32, 0-based), w (None for a unit list), comm, comm16, vweight (None when absent))."""
        r = ResidentGraph()
        self._check(self.L.cge_resident_graph_test(self.h, C.byref(r)))  # (the sizes)
        n, m = r.n, r.m
        src, dst = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        w = None if r.unit or not m else np.empty(m)
        comm = np.empty(n, dtype=np.int32) if r.have & 1 else None
        c16 = np.empty(r.n_comm16, dtype=np.uint16) if r.n_comm16 else None
        vw = np.empty(n) if r.have & 2 else None
        r.src, r.dst, r.w, r.comm, r.comm16, r.vweight = (None if a is None else a.ctypes.data for a in (src, dst, w, comm, c16, vw))
        r.cap_edges, r.cap_vertices, r.cap_comm16 = m, n, r.n_comm16
        self._check(self.L.cge_resident_graph_test(self.h, C.byref(r)))
        return {"n": n, "m": m, "unit": bool(r.unit), "n_comm_max": r.n_comm_max, "src": src, "dst": dst, "w": w, "comm": comm,
                "comm16": c16, "vweight": vw}

    def set_vertex_data(self, comm, vweights):
        cm = None if comm is None else _i64(np.asarray(comm).ravel())
        vw = None if vweights is None else _f64(vweights)
        n = len(cm) if cm is not None else len(vw)
        self._check(self.L.cge_set_vertex_data(self.h, _p(cm), _p(vw), C.c_int64(n)))

    def set_inputs(self, edges, eweights, vweights, comm, embedding):
        n = int(np.asarray(embedding).shape[0])
        self.set_graph(edges, eweights, n)
        self.set_vertex_data(comm, vweights)  # before the embedding: option shard_rows shards the rows BY COMMUNITY
        self.set_embedding(embedding)

    # ---- landmarks ----------------------------------------------------------------------------------
    def landmarks_run(self, clusters, land, forced, method, directed=False):
        flat, off, ncl = _cluster_args(clusters)
        N, ne, tr = C.c_int64(), C.c_int64(), C.c_int()
        self._check(self.L.cge_landmarks_run(self.h, _p(flat), _p(off), C.c_int64(ncl), C.c_int64(land),
                                             C.c_int64(forced), C.c_int(_method_code(method)),
                                             C.c_int(1 if directed else 0), C.byref(N), C.byref(ne), C.byref(tr)))
        self.N, self.n_ledges, self.truncated = N.value, ne.value, bool(tr.value)
        return self.N, self.n_ledges, self.truncated

    def landmarks_info(self):
        N, ne, tr = C.c_int64(), C.c_int64(), C.c_int()
        self._check(self.L.cge_landmarks_info(self.h, C.byref(N), C.byref(ne), C.byref(tr)))
        self.N, self.n_ledges, self.truncated = N.value, ne.value, bool(tr.value)
        return self.N, self.n_ledges, self.truncated

    def landmarks_fetch(self):
        self.landmarks_info()  # sizes come from the library, never from Python-side state
        N, ne, n, d = self.N, self.n_ledges, self.n, self.d
        dii = np.zeros(N)
        embed = np.zeros((N, d), order="F")
        cluster = np.zeros(N, dtype=np.int64)
        ledges = np.zeros((ne, 2), dtype=np.int64, order="F")
        lw = np.zeros(ne)
        lweight = np.zeros(N)
        v_to_l = np.zeros(n, dtype=np.int64)
        self._check(self.L.cge_landmarks_fetch(self.h, _p(dii), _p(embed.ravel(order="K")), _p(cluster),
                                               _p(ledges.ravel(order="K")), _p(lw), _p(lweight), _p(v_to_l)))
        return dii, embed, cluster.reshape(-1, 1), ledges, lw, lweight, v_to_l

    def runsplit(self, clusters, nland, forced, method):
        flat, off, ncl = _cluster_args(clusters)
        out = np.zeros(self.n, dtype=np.int64)
        self._check(self.L.cge_runsplit(self.h, _p(flat), _p(off), C.c_int64(ncl), C.c_int64(nland),
                                        C.c_int64(forced), C.c_int(_method_code(method)), _p(out)))
        return out

    # ---- samples ---------------------------------------------------------------------------------------
    def draw_samples(self, seed, S, directed=False, stream_id=0):
        pos = np.zeros(S, dtype=np.int64)
        ni = np.zeros(S, dtype=np.int64)
        nj = np.zeros(S, dtype=np.int64)
        self._check(self.L.cge_draw_samples(self.h, C.c_int64(seed), C.c_int64(stream_id), C.c_int64(S),
                                            C.c_int(1 if directed else 0), _p(pos), _p(ni), _p(nj)))
        return pos, ni, nj

    # ---- wGCL ------------------------------------------------------------------------------------------
    def wgcl(self, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
             init_eweights, init_embed, split, seed=-1, auc_samples=10000, verbose=False, directed=False,
             samples=None, use_resident_original=False):
        keep = []
        s, t = _edge_cols(edges)
        ew = _f64(eweights)
        cm = _i64(np.asarray(comm).ravel())
        em, emf = _colmajor(embed)
        dist = _f64(distances)
        vw = _f64(vweights)
        ivw = _f64(init_vweights)
        v2l = _i64(v_to_l)
        a = WgclArgs()
        a.edges_src, a.edges_dst, a.eweights, a.m = _p(s).value, _p(t).value, _p(ew).value, len(s)
        a.comm, a.n_comm = _p(cm).value, len(cm)
        a.embed, a.embed_rows, a.d = _p(emf).value, em.shape[0], em.shape[1]
        a.distances, a.n_distances = _p(dist).value, len(dist)
        a.vweights = _p(vw).value
        a.init_vweights, a.n_init = (_p(ivw).value if len(ivw) else None), len(ivw)
        a.v_to_l, a.n_v_to_l = (_p(v2l).value if len(v2l) else None), len(v2l)
        if len(v2l) and not use_resident_original:
            is_, it_ = _edge_cols(init_edges)
            iew = _f64(init_eweights)
            iem, iemf = _colmajor(init_embed)
            keep += [is_, it_, iew, iem, iemf]
            a.init_edges_src, a.init_edges_dst, a.m_init = _p(is_).value, _p(it_).value, len(is_)
            a.init_eweights, a.init_embed = _p(iew).value, _p(iemf).value
        a.split, a.seed, a.auc_samples = int(bool(split)), int(seed), int(auc_samples)
        a.verbose, a.directed = int(bool(verbose)), int(bool(directed))
        if samples is not None:
            arrs = [np.ascontiguousarray(np.atleast_2d(x), dtype=np.int64) for x in samples[:3]]
            keep += arrs
            a.pos_idx, a.neg_i, a.neg_j = (_p(x).value for x in arrs)
            a.n_sample_sets, a.auc_samples = arrs[0].shape
            if len(samples) > 3 and samples[3] is not None:
                p2 = np.ascontiguousarray(np.atleast_2d(samples[3]), dtype=np.int64)
                keep.append(p2)
                a.pos_idx2 = _p(p2).value
        out = np.zeros(7)
        olen = C.c_int(7)
        tr = Trace()
        self._check(self.L.cge_wgcl(self.h, C.byref(a), _p(out), C.byref(olen), C.byref(tr)))
        self.last_trace = tr.as_dict()
        del keep
        return out[: olen.value].copy()

    def score(self, clusters, land, forced=4, method="rss", directed=False, split=False, seed=-1, auc_samples=10000):
        """example/CGE_CLI.jl:10-24 on the resident inputs; land = -1 => exact mode."""
        flat, off, ncl = _cluster_args(clusters)
        a = ScoreArgs()
        a.clusters_flat, a.clusters_off, a.n_clusters = getattr(_p(flat), "value", None), getattr(_p(off), "value", None), ncl
        a.land, a.forced, a.method = int(land), int(forced), _method_code(method)
        a.directed, a.split, a.seed, a.auc_samples = int(bool(directed)), int(bool(split)), int(seed), int(auc_samples)
        out = np.zeros(7)
        olen = C.c_int(7)
        tr = Trace()
        self._check(self.L.cge_score(self.h, C.byref(a), _p(out), C.byref(olen), C.byref(tr)))
        self.last_trace = tr.as_dict()
        return out[: olen.value].copy()

    def score_batch(self, embeddings, clusters, land, forced=4, method="rss", directed=False, split=False, seed=-1,
                    auc_samples=10000, d=None, row_major=True):
        """`score` for K embeddings of the resident graph in one call (cge_score_batch): a list of the K result vectors, each
        equal to what `score` gives on that embedding; their traces in `last_traces`.  `embeddings`: a list of (n, d) float64
        arrays, a (K, n, d) array, or a list of device pointers (ints, as `set_embedding_device`; then `d` is required).
        Afterwards the last embedding is the resident one."""
        if isinstance(embeddings, np.ndarray) and embeddings.ndim == 3:
            embeddings = list(embeddings)
        embeddings = list(embeddings)
        K = len(embeddings)
        if K < 1:
            raise ValueError("score_batch: no embeddings")
        on_device = all(isinstance(e, (int, np.integer)) for e in embeddings)
        keep = []
        if on_device:
            if d is None:
                raise ValueError("score_batch: device pointers need d")
            ptrs = (C.c_void_p * K)(*[int(e) for e in embeddings])
        else:
            for e in embeddings:
                e, ef = _colmajor(e)
                keep.append(ef)
                if e.ndim != 2 or (d is not None and e.shape[1] != d):
                    raise ValueError("score_batch: every embedding is (n, d) with one common d")
                d = e.shape[1]
            ptrs = (C.c_void_p * K)(*[ef.ctypes.data for ef in keep])
        b = EmbeddingBatch()
        b.embeddings = C.cast(ptrs, C.c_void_p).value
        b.K, b.d, b.on_device, b.row_major = K, int(d), int(on_device), int(bool(row_major) and on_device)
        flat, off, ncl = _cluster_args(clusters)
        a = ScoreArgs()
        a.clusters_flat, a.clusters_off, a.n_clusters = getattr(_p(flat), "value", None), getattr(_p(off), "value", None), ncl
        a.land, a.forced, a.method = int(land), int(forced), _method_code(method)
        a.directed, a.split, a.seed, a.auc_samples = int(bool(directed)), int(bool(split)), int(seed), int(auc_samples)
        out = np.zeros((K, 7))
        olen = (C.c_int * K)()
        trs = (Trace * K)()
        self._check(self.L.cge_score_batch(self.h, C.byref(a), C.byref(b), _p(out), olen, trs))
        self.d = int(d)
        self.last_traces = [trs[k].as_dict() for k in range(K)]
        return [out[k, : olen[k]].copy() for k in range(K)]

    def score_views(self, embeddings, clusters, land, forced=4, method="rss", directed=False, split=False, seed=-1,
                    auc_samples=10000):
        """`score_batch` with every member passed as `set_embedding_view` takes it (cge_score_views): the members may differ in
        width, dtype, layout and location -- numpy arrays and torch tensors, host and GPU, mixed.  Returns the list of result
        vectors, each equal to what `set_embedding_view` + `score` gives on that member; traces in `last_traces`.  Afterwards
        the last embedding is the resident one."""
        embeddings = list(embeddings)
        K = len(embeddings)
        if K < 1:
            raise ValueError("score_views: no embeddings")
        views, keep = (EmbeddingView * K)(), []
        for k, e in enumerate(embeddings):
            v, owner = self._view(e)
            if owner.shape[0] != self.n:
                raise ValueError(f"score_views: embedding {k} has {owner.shape[0]} rows, the resident graph {self.n} vertices")
            views[k] = v
            keep.append(owner)
        flat, off, ncl = _cluster_args(clusters)
        a = ScoreArgs()
        a.clusters_flat, a.clusters_off, a.n_clusters = getattr(_p(flat), "value", None), getattr(_p(off), "value", None), ncl
        a.land, a.forced, a.method = int(land), int(forced), _method_code(method)
        a.directed, a.split, a.seed, a.auc_samples = int(bool(directed)), int(bool(split)), int(seed), int(auc_samples)
        out = np.zeros((K, 7))
        olen = (C.c_int * K)()
        trs = (Trace * K)()
        self._check(self.L.cge_score_views(self.h, C.byref(a), views, C.c_int64(K), _p(out), olen, trs))
        self.d = int(views[K - 1].d)
        self.last_traces = [trs[k].as_dict() for k in range(K)]
        del keep
        return [out[k, : olen[k]].copy() for k in range(K)]

    # ---- kernel-level ----------------------------------------------------------------------------------
    def edge_scatter(self, v_to_l, N, Cn, directed=False, e0=0, e1=None, want_wedges=True, want_vect_c=True):
        e1 = self.m if e1 is None else e1
        v2l = None if v_to_l is None else _i64(v_to_l)
        wed = np.zeros((N, N)) if want_wedges else None
        vlen = Cn * Cn if directed else Cn * (Cn + 1) // 2
        vc = np.zeros(vlen) if want_vect_c else None
        self._check(self.L.cge_edge_scatter(self.h, _p(v2l), C.c_int64(N), C.c_int64(Cn), C.c_int(int(directed)),
                                            C.c_int64(e0), C.c_int64(e1), _p(wed), _p(vc)))
        return wed, vc

    def max_pair_dist(self, part=0, nparts=1):
        hi, ai, aj = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self.L.cge_max_pair_dist(self.h, C.c_int(part), C.c_int(nparts), C.byref(hi), C.byref(ai),
                                             C.byref(aj)))
        return hi.value, ai.value, aj.value

    def group_eig(self, A):
        """Testing hook (include/cge_hip_testing.h): principal eigenvectors of a (T, d, d) stack of symmetric
        matrices by the batched device solver of the landmark phase (replaces `eigvecs(A)[:, end]`)."""
        A = _f64(A)
        T, d = A.shape[0], A.shape[1]
        v = np.empty((T, d), dtype=np.float64)
        self._check(self.L.cge_group_eig(self.h, _p(A), C.c_int64(T), C.c_int64(d), _p(v)))
        return v

    def group_stats_test(self, ids, offsets, side=None, mean_in=None):
        """Testing hook (include/cge_hip_testing.h: cge_group_stats_test): the statistics stage of a landmark split for groups of
        the resident rows (0-based ids back to back, offsets (T + 1,)) by the split's own batch builder and launch wrappers.
        mean_in (T, d): the groups' means are given (gathered, not computed; sw is NaN then).  side (R,) of 0 / 1 / 2: also the
        side sums.  Returns a dict: mean (T, d), sw (T,), cov (T, d, d), vec (T, d), z (R,), sums (T, 2, 2 d + 1) or None."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        T, d = off.size - 1, self.d
        assert T >= 1 and off[0] == 0 and off[-1] == ids.size
        mean, sw, cov = np.empty((T, d)), np.full(T, np.nan), np.empty((T, d, d))
        vec, z, sums = np.empty((T, d)), np.empty(ids.size), None
        if side is not None:
            side = np.ascontiguousarray(side, dtype=np.uint8)
            assert side.shape == ids.shape
            sums = np.empty((T, 2, 2 * d + 1))
        if mean_in is not None:
            mean_in = _f64(mean_in)
            assert mean_in.shape == (T, d)
        self._check(self.L.cge_group_stats_test(self.h, _p(ids), _p(off), C.c_int64(T), _p(side), _p(mean_in), _p(mean), _p(sw),
                                                _p(cov), _p(vec), _p(z), _p(sums)))
        return {"mean": mean, "sw": sw, "cov": cov, "vec": vec, "z": z, "sums": sums}

    def group_cut_test(self, ids, offsets, method, z=None, force_generic=False):
        """Testing hook (include/cge_hip_testing.h: cge_group_cut_test): the cut stage of a landmark split for groups of at least
        3 resident rows (0-based ids back to back, offsets (T + 1,)) by rule `method` (a CGE_METHOD_* code) on the projections z
        (R,), or behind the statistics stage when z is None.  Returns a dict: rc (T,), nlow (T,), children (R,), vlow (T,),
        vhigh (T,), cmeans (T, 2, d), route (T,), ties."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        T, d = off.size - 1, self.d
        assert T >= 1 and off[0] == 0 and off[-1] == ids.size
        if z is not None:
            z = _f64(z)
            assert z.shape == ids.shape
        rc, nlow, children = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32), np.full(ids.size, -1, dtype=np.int32)
        vlow, vhigh, cmeans = np.zeros(T), np.zeros(T), np.full((T, 2, d), np.nan)
        route, ties = np.zeros(T, dtype=np.int32), C.c_int32()
        self._check(self.L.cge_group_cut_test(self.h, _p(ids), _p(off), C.c_int64(T), C.c_int(int(method)), _p(z),
                                              C.c_int(1 if force_generic else 0), _p(rc), _p(nlow), _p(children), _p(vlow),
                                              _p(vhigh), _p(cmeans), _p(route), C.byref(ties)))
        return {"rc": rc, "nlow": nlow, "children": children, "vlow": vlow, "vhigh": vhigh, "cmeans": cmeans, "route": route,
                "ties": ties.value}

    def diameter_bounds_test(self, v_to_l, N, lcomm, C_, pass_):
        """Testing hook: the bound matrix of the pruned diameter for a landmark assignment (1-based ids) by one named pass
        (0 fp64, 1 f32, 2 bf16 split).  Returns (P (N, nref), pass that ran, reference points (nref, d), centring mean (d,))."""
        v2l, lc = _i64(v_to_l), _i64(lcomm)
        w = int(C_) if C_ >= 32 else int(N)  # the number of reference points (include/cge_hip_testing.h)
        P, ref, mean = np.zeros((N, w)), np.zeros((w, self.d)), np.zeros(self.d)
        nref, ran = C.c_int64(), C.c_int()
        self._check(self.L.cge_diameter_bounds_test(self.h, _p(v2l), C.c_int64(N), _p(lc), C.c_int64(C_), C.c_int(pass_), _p(P),
                                                    C.byref(nref), C.byref(ran), _p(ref), _p(mean)))
        assert nref.value == w
        return P, ran.value, ref, mean

    def ref_dist2_test(self, refs):
        """Testing hook (cge_ref_dist2_test): the squared distances of the reference points `refs` (nref, d) as the pruned
        diameter forms them.  Returns (rd2 (nref, nref), centring mean (d,))."""
        refs = _f64(refs)
        assert refs.ndim == 2 and refs.shape[1] == self.d
        nref = refs.shape[0]
        rd2, mean = np.zeros((nref, nref)), np.zeros(self.d)
        self._check(self.L.cge_ref_dist2_test(self.h, _p(refs), C.c_int64(nref), _p(rd2), _p(mean)))
        return rd2, mean

    def landmark_graph_test(self, v_to_l, N, directed=False, wedge_form=0, part=0, nparts=1, aggregate=False, wedges=True,
                            positive=None, degrees=False, world=0):
        """Testing hook (include/cge_hip_testing.h: cge_landmark_graph_test): the landmark graph of the assignment v_to_l (n ids
        in 1..N) over the resident inputs, by the landmark run's own aggregate, scatter and degree steps.  aggregate: lemb (N, d),
        lweight, dii, lcomm (0-based).  wedges: the (N, N) landmark-pair matrix of share `part` of `nparts` by wedge_form (0 what
        a run picks, 1 tiled, 2 gather + count); positive (default: with wedges): the count of its positive entries.  degrees: deg_out, deg_in, star from the matrix.  world > 0:
        deg_block (world, 3 N) and u_deg_out, u_deg_in, u_star (the unpacked sum of the blocks).  Returns a dict of what was
        asked for, with form_ran, n_chunks, rshift, colbits, ntile."""
        v2l = _i64(v_to_l)
        N = int(N)
        io, out = LandmarkGraphIO(), {}
        io.v2l, io.N, io.directed, io.wedge_form = v2l.ctypes.data, N, int(bool(directed)), int(wedge_form)
        io.part, io.nparts, io.world = int(part), int(nparts), int(world)

        def want(key, shape, dtype=np.float64):
            out[key] = np.full(shape, -1 if dtype != np.float64 else np.nan, dtype=dtype)
            setattr(io, key, out[key].ctypes.data)

        if aggregate:
            d = getattr(self, "d", 1)  # (no embedding was set through this object: the call refuses)
            want("lemb", (N, d)), want("lweight", N), want("dii", N), want("lcomm", N, np.int32)
        positive = bool(wedges) if positive is None else positive
        if wedges:
            want("wedges", (N, N))
        if positive:
            want("positive", 1, np.int64)
        if degrees:
            want("deg_out", N), want("deg_in", N), want("star", N, np.int32)
        if world:
            want("deg_block", (world, 3 * N)), want("u_deg_out", N), want("u_deg_in", N), want("u_star", N, np.int32)
        self._check(self.L.cge_landmark_graph_test(self.h, C.byref(io)))
        if positive:
            out["positive"] = int(out["positive"][0])
        out.update(form_ran=int(io.form_ran), n_chunks=int(io.n_chunks), rshift=int(io.rshift), colbits=int(io.colbits),
                   ntile=int(io.ntile))
        return out

    def pow_test(self, x, alpha, method):
        """Testing hook: (1 - x)^alpha on the device; method 0 = library pow, 1 = the sweep's exp2(alpha * log2(1 - x))."""
        x = _f64(x)
        out = np.empty_like(x)
        self._check(self.L.cge_pow_test(self.h, _p(x), C.c_int64(x.size), C.c_double(alpha), C.c_int(method), _p(out)))
        return out

    def packed_gd_test(self, emb, diag, alpha, pow_method):
        """Testing hook (include/cge_hip_testing.h: cge_packed_gd_test): the packed form's extrema pass and generator on an
        embedding (N, d) with `diag` on the diagonal of D.  Returns ((lo, hi), GD (N, N)): GD is written for j >= i and inside
        the diagonal 64 x 64 tiles; everything else stays NaN."""
        emb, diag = _f64(emb), _f64(diag)
        N, d = emb.shape
        assert diag.shape == (N,)
        lo_hi, GD = np.zeros(2), np.full((N, N), np.nan)
        self._check(self.L.cge_packed_gd_test(self.h, _p(emb), _p(diag), C.c_int64(N), C.c_int64(d), C.c_double(alpha),
                                              C.c_int(pow_method), _p(lo_hi), _p(GD)))
        return lo_hi, GD

    def vect_b_test(self, GD, Ta, Tb, comm, C_, directed=False, form=0, landmarks=False, vC=None, n_modes=1, second=None,
                    vB=None):
        """Testing hook (include/cge_hip_testing.h: cge_vect_b_test): vect_B of one problem by a named form of the sweep
        (0 = what a sweep of this shape picks) and, with vC, its divergence by the device-side modes.  `second`: the
        (GD, Ta, Tb, comm, C[, vC]) of form 6's other problem.  GD = None with vB and vC: the "JS only" mode.
        Returns a dict: form_ran, vectB, guard (the doubles behind the vector on the device: all NaN unless something wrote
        past its end), js_dev (3,), js_fused (n_modes,) for forms 5 and 6; second_* for form 6's other problem.  Form 7: directed,
        tiles + bins on the packed upper tiles of a symmetric GD."""
        keep, out = [], {}

        def problem(GD, Ta, Tb, comm, C_, vC, vB, tag):
            C_ = int(C_)
            ln = C_ * C_ if directed else C_ * (C_ + 1) // 2
            q = VectBProblem()
            if GD is not None:
                GD, Ta, Tb, comm = _f64(GD), _f64(Ta), _f64(Tb), _i64(comm)
                q.N = GD.shape[0]
                assert GD.shape == (q.N, q.N) and Ta.shape == Tb.shape == comm.shape == (q.N,)
                vect = np.zeros(ln + VECT_B_GUARD)
                q.GD, q.Ta, q.Tb, q.comm = (a.ctypes.data for a in (GD, Ta, Tb, comm))
            else:
                vect = _f64(vB).copy()
                q.N = C_
                assert vect.shape == (ln,) and vC is not None
            q.C = C_
            js_dev, js_fused = np.full(3, np.nan), np.full(2, np.nan)
            if vC is not None:
                vC = _f64(vC)
                assert vC.shape == (ln,)
                q.vC = vC.ctypes.data
            q.vectB, q.js_dev, q.js_fused = vect.ctypes.data, js_dev.ctypes.data, js_fused.ctypes.data
            keep.extend((GD, Ta, Tb, comm, vC, vect, js_dev, js_fused))
            out[tag + "vectB"], out[tag + "guard"] = vect[:ln], vect[ln:]
            out[tag + "js_dev"], out[tag + "js_fused"] = js_dev, js_fused[:n_modes]
            return q

        p1 = problem(GD, Ta, Tb, comm, C_, vC, vB, "")
        p2 = None
        if second is not None:
            p2 = problem(*second[:5], second[5] if len(second) > 5 else None, None, "second_")
        ran = C.c_int(-1)
        self._check(self.L.cge_vect_b_test(self.h, C.byref(p1), C.byref(p2) if p2 is not None else None, C.c_int(int(directed)),
                                           C.c_int(form), C.c_int(int(landmarks)), C.c_int(n_modes), C.byref(ran)))
        out["form_ran"] = ran.value
        return out

    def fit_test(self, problems, directed=False, form=0, eps=None, delta=0.001, want_GD=False):
        """Testing hook (include/cge_hip_testing.h: cge_fit_test): one Chung-Lu fit per problem from a chosen start by a named
        form of the sweep (0 = what an exact-mode sweep of the shape picks).  A problem is a dict: D (N, N), alpha, w, T0
        (undirected) or D, alpha, w = deg_in, w2 = deg_out, T0 = Tin, T0b = Tout (directed); several problems are form 5
        (undirected) or form 6 (directed) only.  Forms 7 / 8: directed, one launch pair per iteration by the tile kernels on the
        row-major GD / on the packed tiles.
        eps defaults to the sweep's (0.25 undirected, 0.9 directed).  Returns (form_ran, [dict(T, Tb, GD, iters, status)]): Tb
        and GD are None where they do not apply / were not asked for."""
        if isinstance(problems, dict):
            problems = [problems]
        n = len(problems)
        arr = (FitProblem * n)()
        keep, outs = [], []
        for q, pr in zip(arr, problems):
            D = _f64(pr["D"])
            N = D.shape[0]
            assert D.shape == (N, N)
            w, T0 = _f64(pr["w"]), _f64(pr["T0"])
            assert w.shape == T0.shape == (N,)
            T = np.full(N, np.nan)
            q.D, q.w, q.T0, q.T, q.N, q.alpha = D.ctypes.data, w.ctypes.data, T0.ctypes.data, T.ctypes.data, N, float(pr["alpha"])
            out = {"T": T, "Tb": None, "GD": None}
            if directed:
                w2, T0b, Tb = _f64(pr["w2"]), _f64(pr["T0b"]), np.full(N, np.nan)
                assert w2.shape == T0b.shape == (N,)
                q.w2, q.T0b, q.Tb = w2.ctypes.data, T0b.ctypes.data, Tb.ctypes.data
                out["Tb"] = Tb
                keep.extend((w2, T0b))
            if want_GD:
                out["GD"] = np.full((N, N), np.nan)
                q.GD = out["GD"].ctypes.data
            q.iters, q.status = -1, -1
            keep.extend((D, w, T0))
            outs.append(out)
        ran = C.c_int(-1)
        eps = (0.9 if directed else 0.25) if eps is None else eps
        self._check(self.L.cge_fit_test(self.h, arr, C.c_int(n), C.c_int(int(directed)), C.c_int(form), C.c_double(eps),
                                        C.c_double(delta), C.byref(ran)))
        for q, out in zip(arr, outs):
            out["iters"], out["status"] = int(q.iters), int(q.status)
        return ran.value, outs

    def fused_chain_test(self, problems, directed=False, eps=0.25, delta=0.001):
        """Testing hook (include/cge_hip_testing.h: cge_fused_chain_test): one alpha of the fused chain per problem -- the fused
        fit with its epilogue's outputs, the bins, the divergence; one problem by fit_flow_kernel, several by one
        fit_flow_multi_kernel launch.  A problem is a dict: D (N, N), alpha, w, T0, comm (ids in 1..C), C, want (bit 0 vect_B's
        partials, bit 1 the tallies), optional vC with n_modes, and with want bit 1 `tally` = dict(aidx (4, S), afac (8, S),
        aden (64,), dpos, dneg, wts (S,)).  Returns a list of dicts: T, iters, status, order, fc, ns, base, bt_total, partials
        (bt_total,), vectB, guard, js_fused (n_modes,), part (64, 2), apw (2, S) or None."""
        if isinstance(problems, dict):
            problems = [problems]
        n = len(problems)
        arr = (FusedChainProblem * n)()
        keep, outs = [], []
        for q, pr in zip(arr, problems):
            D, w, T0, comm = _f64(pr["D"]), _f64(pr["w"]), _f64(pr["T0"]), _i64(pr["comm"])
            N, C_ = D.shape[0], int(pr["C"])
            assert D.shape == (N, N) and w.shape == T0.shape == comm.shape == (N,)
            Nt, ln = (N + 63) // 64, C_ * (C_ + 1) // 2
            q.D, q.w, q.T0, q.comm = (a.ctypes.data for a in (D, w, T0, comm))
            q.N, q.C, q.alpha, q.want, q.n_modes = N, C_, float(pr["alpha"]), int(pr["want"]), int(pr.get("n_modes", 1))
            o = {"T": np.full(N, np.nan), "order": np.full(N, -1, np.int32), "fc": np.full(Nt, -1, np.int32),
                 "ns": np.full(Nt, -1, np.int32), "base": np.full(Nt * Nt, -1, np.int32),
                 # (a block spans at most min(64, C) ids: no layout has more partials)
                 "partials": np.full(Nt * (Nt + 1) // 2 * min(64, max(C_, 1)) ** 2, np.nan),
                 "vectB": np.full(max(ln, 0) + VECT_B_GUARD, np.nan), "js_fused": np.full(2, np.nan),
                 "part": np.full((64, 2), np.nan), "apw": None}
            q.T, q.order, q.fc, q.ns, q.base = (o[k].ctypes.data for k in ("T", "order", "fc", "ns", "base"))
            q.partials, q.partials_cap = o["partials"].ctypes.data, o["partials"].size
            q.vectB, q.js_fused, q.part = o["vectB"].ctypes.data, o["js_fused"].ctypes.data, o["part"].ctypes.data
            if pr.get("vC") is not None:
                vC = _f64(pr["vC"])
                assert vC.shape == (ln,)
                q.vC = vC.ctypes.data
                keep.append(vC)
            if pr.get("tally") is not None:
                t = pr["tally"]
                aidx = np.ascontiguousarray(t["aidx"], dtype=np.int32)
                afac, aden, dpos, dneg, wts = (_f64(t[k]) for k in ("afac", "aden", "dpos", "dneg", "wts"))
                S = dpos.shape[0]
                assert aidx.shape == (4, S) and afac.shape == (8, S) and aden.shape == (64,) and dneg.shape == wts.shape == (S,)
                o["apw"] = np.full((2, S), np.nan)
                q.S, q.aidx, q.afac, q.aden, q.dpos, q.dneg, q.wts, q.apw = (S, aidx.ctypes.data, afac.ctypes.data, aden.ctypes.data,
                                                                          dpos.ctypes.data, dneg.ctypes.data, wts.ctypes.data,
                                                                          o["apw"].ctypes.data)
                keep.extend((aidx, afac, aden, dpos, dneg, wts))
            q.iters, q.status, q.bt_total = -1, -1, -1
            keep.extend((D, w, T0, comm))
            outs.append(o)
        self._check(self.L.cge_fused_chain_test(self.h, arr, C.c_int(n), C.c_int(int(directed)), C.c_double(eps), C.c_double(delta)))
        for q, pr, o in zip(arr, problems, outs):
            ln = int(pr["C"]) * (int(pr["C"]) + 1) // 2
            o["iters"], o["status"], o["bt_total"] = int(q.iters), int(q.status), int(q.bt_total)
            o["partials"] = o["partials"][:o["bt_total"]]
            o["vectB"], o["guard"] = o["vectB"][:ln], o["vectB"][ln:]
            o["js_fused"] = o["js_fused"][:int(q.n_modes)]
        return outs

    def sweep_setup_test(self, emb, dist, comm, C_, vw=None, directed=False, landmarks=False, force_relabel=False, log_form=0,
                         alpha=None, edges=None, want=("layout", "D_raw", "D", "log", "start")):
        """Testing hook (include/cge_hip_testing.h: cge_sweep_setup_test): the set-up of an alpha sweep on the score graph emb
        (N, d), dist (N,), comm (ids in 1..C_), optional vw -- no fit runs.  edges = (src, dst, w or None), 0-based: the
        directed degree pass (a directed call needs it).  `want` names the stages whose outputs come back: "layout" (relabel,
        order, old2new, emb_rl, vec_rl (4, N), comm_rl, cm_off, cm_mem, cm_pos), "D_raw", "D" (lo_hi, D), "log" (Lh, Ll,
        log_form_ran, log_count), "start" (T1, T2, TT (3, Tld), Tld); the degrees (deg_out, deg_in, star) come with edges, GD with
        alpha.  Arrays nothing wrote keep their fill: NaN, or -1 for the integers."""
        emb, dist, comm = _f64(emb), _f64(dist), _i64(comm)
        N, d = emb.shape
        assert dist.shape == comm.shape == (N,)
        io, out, keep = SweepSetupIO(), {}, [emb, dist, comm]
        io.emb, io.dist, io.comm = emb.ctypes.data, dist.ctypes.data, comm.ctypes.data
        io.N, io.d, io.C = N, d, int(C_)
        io.directed, io.landmarks, io.force_relabel, io.log_form = int(bool(directed)), int(bool(landmarks)), int(bool(force_relabel)), int(log_form)

        def give(key, a, dtype):
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            setattr(io, key, a.ctypes.data)
            return a

        def ask(key, shape, dtype=np.float64):
            out[key] = np.full(shape, -1 if dtype == np.int32 else np.nan, dtype=dtype)
            setattr(io, key, out[key].ctypes.data)

        if vw is not None:
            assert give("vw", vw, np.float64).shape == (N,)
        if edges is not None:
            src = give("src", edges[0], np.int32)
            assert give("dst", edges[1], np.int32).shape == src.shape and src.ndim == 1
            if edges[2] is not None:
                assert give("w", edges[2], np.float64).shape == src.shape
            io.m = src.size
            ask("deg_out", N), ask("deg_in", N), ask("star", N, np.int32)
        n_out, Nt = max(N, 1), (max(N, 1) + 63) // 64
        if "layout" in want:
            for key in ("order", "old2new", "comm_rl", "cm_mem", "cm_pos"):
                ask(key, n_out, np.int32)
            ask("cm_off", max(int(C_), 0) + 1, np.int32), ask("emb_rl", (n_out, max(d, 1))), ask("vec_rl", (4, n_out))
        if "D_raw" in want:
            ask("D_raw", (n_out, n_out))
        if "D" in want:
            ask("lo_hi", 2), ask("D", (n_out, n_out))
        if "log" in want:
            io.log_cap = max(n_out * n_out, Nt * (Nt + 1) // 2 * 4096)
            ask("Lh", io.log_cap), ask("Ll", io.log_cap, np.float32)
        if alpha is not None:
            io.alpha = float(alpha)
            ask("GD", (n_out, n_out))
        if "start" in want:
            ask("T1", n_out), ask("T2", n_out), ask("TT", (3, 64 * Nt))
        self._check(self.L.cge_sweep_setup_test(self.h, C.byref(io)))
        out["relabel"], out["Tld"] = int(io.relabel), int(io.Tld)
        if "log" in want:
            out["log_form_ran"], out["log_count"] = int(io.log_form_ran), int(io.log_count)
            out["Lh"], out["Ll"] = out["Lh"][:io.log_count], out["Ll"][:io.log_count]
        return out

    def local_score_test(self, S, directed=False, draw=None, draws=None, pos2=None, pairs=None, prepare=False, hi=None,
                         distances=False, dists=None, tally=None, sharded=False):
        """Testing hook (include/cge_hip_testing.h: cge_local_score_test): the stages of the local score on the resident graph
        and embedding; every id is 0-based.
          draw = (seed, stream_id, route): the device sampler (route 1 k_draw_samples_dev, 2 _begin + _finish) -> pos, neg_i,
            neg_j, attempt, rounds;
          draws = (pos, neg_i, neg_j), pos2: supplied draws for Prepare; prepare=True -> pi, pj, ni, nj, wts;
          pairs = (pi, pj, ni, nj, wts): supplied pairs in place of Prepare; hi with distances=True -> dpos, dneg;
          dists = (dpos, dneg): supplied distances for the tally;
          tally = dict(form (5: k_auc_exact on the packed tiles with ordered pairs), N, alpha, Ta, Tb, v2l, vw, lweight, old2new, GD, D, w, T0, eps, delta) -> part (64, 2), out2 and,
            form 4, T, aidx (4, S), afac (8, S), aden (64,), iters, status.
          sharded=True: the opt-in of a context whose rows or edges are sharded over ranks -- Draw, Prepare and Distances run
            collectively (every rank calls with the same arguments; ids stay global); the tally forms stay refused there.
        Returns a dict of what the stages that were asked for give."""
        S = int(S)
        io, out, keep = LocalScoreIO(), {}, []
        io.S, io.directed, io.sharded = S, int(bool(directed)), int(bool(sharded))

        def give(key, a, dtype):
            if a is None:
                return
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            setattr(io, key, a.ctypes.data)

        def want(key, shape, dtype=np.float64):
            fill = np.nan if dtype == np.float64 else -1 if dtype == np.int32 else np.iinfo(dtype).max
            out[key] = np.full(shape, fill, dtype=dtype)
            setattr(io, key, out[key].ctypes.data)

        n_out = max(S, 1)
        if draw is not None:
            io.seed, io.stream_id, io.draw_route = int(draw[0]), int(draw[1]), int(draw[2])
            want("pos", n_out, np.int32), want("neg_i", n_out, np.int32), want("neg_j", n_out, np.int32)
            want("attempt", n_out, np.uint32)
        if draws is not None:
            for key, a in zip(("pos_in", "neg_i_in", "neg_j_in"), draws):
                give(key, a, np.int32)
        give("pos2_in", pos2, np.int32)
        if prepare:
            for key in ("pi", "pj", "ni", "nj"):
                want(key, n_out, np.int32)
            want("wts", n_out)
        if pairs is not None:
            for key, a in zip(("pi_in", "pj_in", "ni_in", "nj_in"), pairs[:4]):
                give(key, a, np.int32)
            give("wts_in", pairs[4], np.float64)
        if hi is not None:
            io.hi = float(hi)
        if distances:
            want("dpos", n_out), want("dneg", n_out)
        if dists is not None:
            give("dpos_in", dists[0], np.float64), give("dneg_in", dists[1], np.float64)
        if tally is not None:
            t = dict(tally)
            io.form, io.N, io.alpha = int(t.pop("form")), int(t.pop("N")), float(t.pop("alpha", 1.0))
            io.eps, io.delta = float(t.pop("eps", 0.25)), float(t.pop("delta", 0.001))
            for key in ("v2l", "old2new"):
                give(key, t.pop(key, None), np.int32)
            for key in ("Ta", "Tb", "vw", "lweight", "GD", "D", "w", "T0"):
                give(key, t.pop(key, None), np.float64)
            assert not t, sorted(t)
            want("part", (64, 2)), want("out2", 2)
            if io.form == 4:
                want("T", max(io.N, 1)), want("aidx", (4, n_out), np.int32), want("afac", (8, n_out)), want("aden", 64)
            io.iters, io.status = -1, -1
        self._check(self.L.cge_local_score_test(self.h, C.byref(io)))
        if draw is not None:
            out["rounds"] = int(io.rounds)
        if tally is not None and io.form == 4:
            out["iters"], out["status"] = int(io.iters), int(io.status)
        return out

    def segment_sort_test(self, z, offsets):
        """Testing hook: the per-group stable sort of runsplit's projections; returns (sorted z, local permutation)."""
        z = _f64(z)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        zs, perm = np.empty_like(z), np.empty(z.size, dtype=np.int32)
        self._check(self.L.cge_segment_sort_test(self.h, _p(z), _p(off), C.c_int64(off.size - 1), _p(zs), _p(perm)))
        return zs, perm

    def wave_tree_test(self, x):
        """Testing hook: per row of 64 doubles the shuffle-tree sum and the lane-swap sum of the projection kernel."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 64)
        a, b = np.empty(x.shape[0]), np.empty(x.shape[0])
        self._check(self.L.cge_wave_tree_test(self.h, _p(x), C.c_int64(x.shape[0]), _p(a), _p(b)))
        return a, b

    def js(self, vC, vB, vI=None, internal=True):
        vC, vB = _f64(vC), _f64(vB)
        vi = None if vI is None or len(vI) == 0 else np.ascontiguousarray(vI, dtype=np.uint8)
        out = C.c_double()
        self._check(self.L.cge_js(self.h, _p(vC), _p(vB), C.c_int64(len(vC)), _p(vi), C.c_int(int(bool(internal))),
                                  C.byref(out)))
        return out.value

    # ---- collectives / profiling -----------------------------------------------------------------------
    def exchange_buffer(self, min_doubles):
        ptr, cap = C.c_void_p(), C.c_int64()
        self._check(self.L.cge_exchange_buffer(self.h, C.c_int64(min_doubles), C.byref(ptr), C.byref(cap)))
        return ptr.value, cap.value

    def set_collectives(self, fn, rank, world):
        cb = ALLREDUCE_FN(fn)
        coll = Collectives(cb, None, rank, world)
        self._keep = [cb, coll]
        self._check(self.L.cge_set_collectives(self.h, C.byref(coll)))

    def set_collectives_ext(self, allgather=None, reduce_scatter=None):
        """Optional further ops of the hook (include/cge_hip.h: cge_collectives_ext); call after set_collectives."""
        ag = GATHER_FN(allgather) if allgather else GATHER_FN()
        rs = GATHER_FN(reduce_scatter) if reduce_scatter else GATHER_FN()
        ext = CollectivesExt(ag, rs)
        self._keep = list(getattr(self, "_keep", [])) + [ag, rs, ext]
        self._check(self.L.cge_set_collectives_ext(self.h, C.byref(ext)))

    def clear_collectives(self):
        """Back to a single-rank context: the in-library communicator is released and the hook removed."""
        self._check(self.L.cge_comm_finalize(self.h))
        self._check(self.L.cge_set_collectives(self.h, None))
        self._keep = []

    def init_rccl(self, unique_id: bytes, rank: int, world: int):
        """In-library collectives (include/cge_hip.h: cge_comm_init_rccl): every rank calls this with rank 0's id."""
        assert len(unique_id) == 128
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.L.cge_comm_init_rccl(self.h, buf, C.c_int(rank), C.c_int(world)))

    def finalize_rccl(self):
        """Release the in-library communicator (cge_comm_finalize); collectives go back to the hook, if one is set."""
        self._check(self.L.cge_comm_finalize(self.h))

    def rccl_selftest(self, arr, op=0):
        """Testing hook: all-reduce `arr` (float64, or int64 for op 2) through the context's communicator."""
        a = np.ascontiguousarray(arr).copy()
        assert a.dtype.itemsize == 8
        self._check(self.L.cge_rccl_selftest(self.h, _p(a), C.c_int64(a.size), C.c_int(op)))
        return a

    def louvain(self):
        """Level-1 Louvain communities of the resident graph: (comm 0-based (n,), n_comm, modularity, rounds)."""
        out = np.zeros(self.n, dtype=np.int64)
        nc, q, rounds = C.c_int64(), C.c_double(), C.c_int64()
        self._check(self.L.cge_louvain(self.h, _p(out), C.byref(nc), C.byref(q), C.byref(rounds)))
        return out, nc.value, q.value, rounds.value

    def louvain_levels(self, max_levels=0):
        """The Louvain hierarchy of the resident graph (cge_louvain_levels): a list with one (comm 0-based (n,) of the ORIGINAL
        vertices, n_comm, modularity, rounds) per level; entry 0 is `louvain()`'s result.  max_levels > 0 stops there; otherwise
        the hierarchy ends at the first level that merges nothing (not reported, except level 1)."""
        count, cap = C.c_int64(), (int(max_levels) if 0 < int(max_levels) < 8 else 8)  # (a count-only call would run the whole hierarchy once more; beyond 8 levels it is run again)
        while True:
            comm = np.zeros((cap, self.n), dtype=np.int64)
            nc, q, rounds = np.zeros(cap, dtype=np.int64), np.zeros(cap), np.zeros(cap, dtype=np.int64)
            rc = self.L.cge_louvain_levels(self.h, C.c_int64(int(max_levels)), C.c_int64(cap), _p(comm), C.byref(count), _p(nc),
                                           _p(q), _p(rounds))
            if rc == -7 and count.value > cap:  # CGE_E_ARG that names the count
                cap = count.value
                continue
            self._check(rc)
            break
        return [(comm[l], int(nc[l]), float(q[l]), int(rounds[l])) for l in range(count.value)]

    def ecg(self, members=16, w_min=0.05, seed=0, final_level=-1, edge_weights=False):
        """ECG communities of the resident graph (cge_ecg): `members` relabelled level-1 passes, every edge reweighted by how
        often its ends were co-clustered (w_min off the 2-core), the Louvain hierarchy on those weights.  Returns (comm 0-based
        (n,), n_comm, modularity on the resident graph, modularity on the reweighted graph[, the new weight of every edge (m,)])."""
        args = EcgArgs(int(members), float(w_min), int(seed), int(final_level))
        out = np.zeros(self.n, dtype=np.int64)
        w = np.zeros(self.m) if edge_weights else None
        nc, q, q_ecg = C.c_int64(), C.c_double(), C.c_double()
        self._check(self.L.cge_ecg(self.h, C.byref(args), _p(out), C.byref(nc), C.byref(q), C.byref(q_ecg), _p(w) if edge_weights else None))
        return (out, nc.value, q.value, q_ecg.value) + ((w,) if edge_weights else ())

    # ---- link prediction under the fitted model (cge_link_*) -------------------------------------------
    _LINK_WHICH = {"local": 1, "global": 2}  # CGE_LINK_BEST_LOCAL / CGE_LINK_BEST_GLOBAL

    def link_fit(self, clusters, land, forced=4, method="rss", directed=False, split=False, seed=-1, auc_samples=10000,
                 which="local"):
        """`score` that also keeps the geometric Chung-Lu model of one alpha (cge_link_fit): which = "local" the alpha of element
        5 (best local score), "global" the alpha of element 1 (best divergence).  Returns (vector, trace); both equal `score`'s."""
        if which not in self._LINK_WHICH:
            raise ValueError(f"link_fit: which = {which!r} is neither 'local' nor 'global'")
        flat, off, ncl = _cluster_args(clusters)
        a = ScoreArgs()
        a.clusters_flat, a.clusters_off, a.n_clusters = getattr(_p(flat), "value", None), getattr(_p(off), "value", None), ncl
        a.land, a.forced, a.method = int(land), int(forced), _method_code(method)
        a.directed, a.split, a.seed, a.auc_samples = int(bool(directed)), int(bool(split)), int(seed), int(auc_samples)
        out = np.zeros(7)
        olen = C.c_int(7)
        tr = Trace()
        self._check(self.L.cge_link_fit(self.h, C.byref(a), C.c_int(self._LINK_WHICH[which]), _p(out), C.byref(olen), C.byref(tr)))
        self.last_trace = tr.as_dict()
        return out[: olen.value].copy(), self.last_trace

    def link_set_model(self, alpha, hi, f_out, f_in=None, directed=False):
        """A caller-supplied model over the resident embedding and graph: p(i, j) = f_out[i] f_in[j] max(0, 1 - dist / hi)^alpha
        (f_in = None: f_out)."""
        fo = _f64(_host_array(f_out)).ravel()
        fi = None if f_in is None else _f64(_host_array(f_in)).ravel()
        if fi is not None and len(fi) != len(fo):
            raise ValueError("link_set_model: f_out and f_in differ in length")
        self._check(self.L.cge_link_set_model(self.h, C.c_int(int(bool(directed))), C.c_double(float(alpha)), C.c_double(float(hi)),
                                              _p(fo), _p(fi), C.c_int64(len(fo))))

    def link_model(self):
        """The resident link model: {"directed", "alpha", "hi", "f_out", "f_in", "T_out", "T_in"}; the T's are the landmark (exact
        mode: vertex) iterates of a fitted model, empty for a supplied one."""
        d, alpha, hi, N = C.c_int(), C.c_double(), C.c_double(), C.c_int64()
        self._check(self.L.cge_link_model_fetch(self.h, C.byref(d), C.byref(alpha), C.byref(hi), None, None, None, None, C.byref(N)))
        fo, fi = np.zeros(self.n), np.zeros(self.n)
        To, Ti = np.zeros(N.value), np.zeros(N.value)
        self._check(self.L.cge_link_model_fetch(self.h, None, None, None, _p(fo), _p(fi), _p(To) if N.value else None,
                                                _p(Ti) if N.value else None, None))
        return {"directed": bool(d.value), "alpha": alpha.value, "hi": hi.value, "f_out": fo, "f_in": fi, "T_out": To, "T_in": Ti}

    def link_prob(self, i, j):
        """The model's probability of the pairs (i[q], j[q]): 1-based vertex ids as `draw_samples` returns them (numpy arrays or
        torch tensors, any integer type)."""
        ii, jj = _i64(_host_array(i)).ravel(), _i64(_host_array(j)).ravel()
        if len(ii) != len(jj):
            raise ValueError("link_prob: i and j differ in length")
        out = np.zeros(len(ii))
        self._check(self.L.cge_link_prob(self.h, _p(ii), _p(jj), C.c_int64(len(ii)), _p(out)))
        return out

    def link_topk(self, queries, k, exclude_edges=True):
        """Per query vertex (1-based ids, repeats allowed) the k most probable candidates j != i under the model, sorted by
        (p descending, j ascending); exclude_edges leaves out the query's resident neighbours (directed: its out-neighbours).
        Returns (j (Q, k) 1-based, p (Q, k), count (Q,)); unused slots hold 0 / 0.0."""
        q = _i64(_host_array(queries)).ravel()
        Q, k = len(q), int(k)
        kk = max(k, 1)
        oj, op, oc = np.zeros((Q, kk), dtype=np.int64), np.zeros((Q, kk)), np.zeros(Q, dtype=np.int64)
        self._check(self.L.cge_link_topk(self.h, _p(q), C.c_int64(Q), C.c_int64(k), C.c_int(int(bool(exclude_edges))), _p(oj), _p(op),
                                         _p(oc)))
        return oj, op, oc

    def link_rank(self, i, j, exclude_edges=True):
        """The exact filtered rank of the pairs (i[q], j[q]) (1-based ids) among the candidates of their source vertex
        (cge_link_rank): with p* = `link_prob`'s value of the pair and the candidates c other than i and j -- and, under
        exclude_edges, not a resident neighbour of i -- returns (greater, ties, cand, p): how many candidates have p(i, c) > p*,
        how many have p(i, c) == p*, how many there are, and p*.  All numpy, in the caller's order; see `link_metrics`."""
        ii, jj = _i64(_host_array(i)).ravel(), _i64(_host_array(j)).ravel()
        if len(ii) != len(jj):
            raise ValueError("link_rank: i and j differ in length")
        P = len(ii)
        g, t, cand = (np.zeros(max(P, 1), dtype=np.int64) for _ in range(3))
        p = np.zeros(max(P, 1))
        if P == 0:  # (no pairs: the library says so; it is handed valid pointers all the same)
            ii = jj = np.zeros(1, dtype=np.int64)
        self._check(self.L.cge_link_rank(self.h, _p(ii), _p(jj), C.c_int64(P), C.c_int(int(bool(exclude_edges))), _p(g), _p(t),
                                         _p(cand), _p(p)))
        return g[:P], t[:P], cand[:P], p[:P]

    def _link_sample_call(self, call, cap, want_p):
        """`call(cap, out_i, out_j, out_p, n_edges)` -> rc, with cap = None grown once to the count the library reports."""
        first = cap is None
        cap = 2 * int(self.m) + 16 if first else int(cap)
        while True:
            k = max(cap, 1)
            oi, oj = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
            op = np.zeros(k) if want_p else None
            ne = C.c_int64(-1)
            rc = call(C.c_int64(cap), _p(oi) if cap > 0 else None, _p(oj) if cap > 0 else None,
                      _p(op) if want_p and cap > 0 else None, C.byref(ne))
            if first and rc == -7 and ne.value > cap:  # CGE_E_ARG that names the count
                cap, first = ne.value, False
                continue
            self._check(rc)
            break
        e = ne.value if cap > 0 else 0
        return oi[:e], oj[:e], (op[:e] if want_p else None), ne.value

    def link_sample(self, seed=0, stream=0, cap=None, want_p=False):
        """One draw of the random graph the resident model is (cge_link_sample): the pairs with u(i, j) < p(i, j), u the counter
        stream's uniform of the pair -- i < j of an undirected model, every ordered i != j of a directed one.  Returns (i, j, p or
        None, n_edges): 1-based ids sorted by (i, j).  cap = 0 only counts; cap = None starts from twice the resident edge count
        and asks once more with the reported count; a given cap that is too small raises (the count is in the message)."""
        return self._link_sample_call(
            lambda cap_, oi, oj, op, ne: self.L.cge_link_sample(self.h, C.c_int64(int(seed)), C.c_int64(int(stream)), cap_, oi, oj, op,
                                                                ne), cap, want_p)

    def link_sample_test(self, U, directed_layout=True, cap=None, want_p=False):
        """Testing hook (cge_link_sample_test): `link_sample` with u(a, b) = U[a, b] ((n, n), 0-based, n <= 1024;
        directed_layout = False reads the upper triangle alone) in the place of the counter stream."""
        Um = np.ascontiguousarray(_f64(_host_array(U)))
        if Um.shape != (self.n, self.n):
            raise ValueError(f"link_sample_test: U is {Um.shape}, not ({self.n}, {self.n})")
        return self._link_sample_call(
            lambda cap_, oi, oj, op, ne: self.L.cge_link_sample_test(self.h, _p(Um), C.c_int(int(bool(directed_layout))), cap_, oi, oj,
                                                                     op, ne), cap, want_p)

    def link_auc(self, part=0, nparts=1, want_counts=False, want_p=False):
        """The exact link AUC of the resident model on the resident graph (cge_link_auc): every resident edge row against every
        non-edge.  Returns {"local_exact": 1 - L / (W n_neg) -- what element 5 of a score estimates from samples; ties count
        against --, "auc": (L + Tq / 2) / (W n_neg), "n_pos", "n_neg", "W", "L", "Tq"}; with want_counts also "less" / "ties"
        (int64 (m,), the edge list's order), with want_p also "p".  `part` of `nparts` visits its share of the pair tiles: the
        quotients of a part are of that part's sums (add the parts' counts up and use `link_auc_from_counts`).  No non-edges:
        the quotients are NaN."""
        part, nparts = int(part), int(nparts)
        if nparts < 1 or not 0 <= part < nparts:
            raise ValueError(f"link_auc: part = {part} of nparts = {nparts}")
        m = int(self.m)
        less = np.zeros(max(m, 1), dtype=np.int64) if want_counts else None
        ties = np.zeros(max(m, 1), dtype=np.int64) if want_counts else None
        p = np.zeros(max(m, 1)) if want_p else None
        nneg, summ = C.c_int64(-1), np.zeros(3)
        self._check(self.L.cge_link_auc(self.h, C.c_int(part), C.c_int(nparts), _p(less) if want_counts else None,
                                        _p(ties) if want_counts else None, _p(p) if want_p else None, C.byref(nneg), _p(summ)))
        W, L, Tq = (float(x) for x in summ)
        out = {"n_pos": m, "n_neg": int(nneg.value), "W": W, "L": L, "Tq": Tq}
        out["local_exact"], out["auc"] = _link_auc_quotients(W, L, Tq, nneg.value)
        if want_counts:
            out["less"], out["ties"] = less[:m], ties[:m]
        if want_p:
            out["p"] = p[:m]
        return out

    def link_moments(self, diag=False):
        """The moments of the resident model over every pair, for the resident vertex communities (cge_link_moments): a
        `LinkMoments` with deg_out / deg_in (n; one vector under both names when undirected), B = sum p and V = sum q (1 - q),
        q = min(p, 1), per community bin in the sweep's vect_B layout, C = the sweep's vect_C of the resident edges, n_comm and
        directed.  diag adds the self pairs p(i, i) = f_out[i] f_in[i] as the reference's exact-mode loops do.  Sums within an
        a-priori bound of the real-number values (include/cge_hip.h), and a function of the inputs alone."""
        nc = C.c_int64(-1)
        self._check(self.L.cge_link_moments(self.h, C.c_int(int(bool(diag))), None, None, None, None, None, C.byref(nc)))
        d = C.c_int()
        self._check(self.L.cge_link_model_fetch(self.h, C.byref(d), None, None, None, None, None, None, None))
        directed, nco = bool(d.value), int(nc.value)
        L = nco * nco if directed else nco * (nco + 1) // 2
        do = np.zeros(self.n)
        di = np.zeros(self.n) if directed else do
        B, V, Cobs = np.zeros(L), np.zeros(L), np.zeros(L)
        self._check(self.L.cge_link_moments(self.h, C.c_int(int(bool(diag))), _p(do), _p(di) if directed else None, _p(B), _p(V),
                                            _p(Cobs), C.byref(nc)))
        return LinkMoments(do, di, B, V, Cobs, nco, directed)

    def link_triangles(self, model=True, graph=True):
        """Expected and observed triangles and wedges per vertex (cge_link_triangles; undirected models only).  Returns
        (tri_exp, wed_exp, tri_obs, wed_obs, summary): float64 (n,) twice -- q = min(p, 1) of the resident model, the draws'
        probability --, int64 (n,) twice -- the resident edge list as a simple undirected graph --, and summary = the four sums
        (long double on the host, rounded once).  model = False / graph = False skips that half: its arrays are None and its
        sums 0.  The model half holds an (n padded)^2 matrix of doubles on the device."""
        n = int(self.n)
        te, we = (np.zeros(n), np.zeros(n)) if model else (None, None)
        to, wo = (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)) if graph else (None, None)
        summ = np.zeros(4)
        self._check(self.L.cge_link_triangles(self.h, _p(te) if model else None, _p(we) if model else None,
                                              _p(to) if graph else None, _p(wo) if graph else None, _p(summ)))
        return te, we, to, wo, summ

    def link_triangles_test(self):
        """Testing hook (cge_link_triangles_test): the matrix Q of the model half, (ld, ld) with ld = 128 (ceil(n / 128) | 1),
        n <= 2048."""
        ld = 128 * (((int(self.n) + 127) // 128) | 1)
        Q = np.zeros((ld, ld))
        self._check(self.L.cge_link_triangles_test(self.h, _p(Q), C.c_int64(ld)))
        return Q

    def ecg_members_test(self, members=16, seed=0):
        """Testing hook (cge_ecg_members_test): the member and peel stages of `ecg` alone -- (members (K, n) each renumbered as a
        pass is, n_comm (K,), rounds (K,), modularity (K,), core (n,) bool)."""
        K = int(members)
        mem = np.zeros((max(K, 1), self.n), dtype=np.int64)
        nc, rounds, q = np.zeros(max(K, 1), dtype=np.int64), np.zeros(max(K, 1), dtype=np.int64), np.zeros(max(K, 1))
        core = np.zeros(self.n, dtype=np.int32)
        self._check(self.L.cge_ecg_members_test(self.h, C.c_int64(K), C.c_int64(int(seed)), _p(mem), _p(nc), _p(rounds), _p(q), _p(core)))
        return mem, nc, rounds, q, core.astype(bool)

    _TEST_OPTIONS = ("louvain_wave_len", "fit_persistent_test_delay", "fit_persistent_test_timeout", "test_bvec_plain", "test_rss2_one_kernel",
                     "exact_resident_limit", "test_eig_roles", "fit_dir_tiles", "test_pcent_form", "test_device_cus",
                     "test_lm_speculate")

    def set_option(self, key, value):
        if key in self._TEST_OPTIONS:  # the testing knobs are not part of the boundary (include/cge_hip_testing.h)
            self._check(self.L.cge_set_test_option(self.h, key.encode(), C.c_int64(int(value))))
            return
        self._check(self.L.cge_set_option(self.h, key.encode(), C.c_int64(int(value))))

    def get_stat(self, key):
        v = C.c_int64()
        self._check(self.L.cge_get_stat(self.h, key.encode(), C.byref(v)))
        return v.value

    def last_diameter(self):
        """(hi, path, candidate landmark pairs, candidate tiles) of the last landmark-mode run."""
        import struct

        hi = struct.unpack("d", struct.pack("q", self.get_stat("diameter_bits")))[0]
        return hi, {1: "brute", 2: "pruned"}.get(self.get_stat("diameter_path"), "none"), \
            self.get_stat("diameter_candidate_pairs"), self.get_stat("diameter_candidate_tiles")

    def profile_enable(self, on=True):
        self._check(self.L.cge_profile_enable(self.h, C.c_int(int(on))))

    def profile_select(self, names=()):
        """Time only the named kernels (empty: all) -- every timer is a pair of events on the stream."""
        self._check(self.L.cge_profile_select(self.h, ",".join(names).encode()))

    def profile_reset(self):
        self._check(self.L.cge_profile_reset(self.h))

    def profile(self):
        buf = C.create_string_buffer(4096)
        self._check(self.L.cge_profile_names(self.h, buf, C.c_int64(4096)))
        res = {}
        for name in filter(None, buf.value.decode().split(",")):
            n, ms = C.c_int64(), C.c_double()
            self._check(self.L.cge_profile_get(self.h, name.encode(), C.byref(n), C.byref(ms)))
            res[name] = {"launches": n.value, "total_ms": ms.value}
        return res

    def phase_ms(self):
        res = {}
        buf = C.create_string_buffer(4096)
        self._check(self.L.cge_phase_names(self.h, buf, C.c_int64(4096)))
        for ph in filter(None, buf.value.decode().split(",")):
            ms = C.c_double()
            self._check(self.L.cge_phase_ms(self.h, ph.encode(), C.byref(ms)))
            res[ph] = ms.value
        return res


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def rccl_unique_id() -> bytes:
    """Rank 0: the 128-byte id every rank passes to Context.init_rccl (include/cge_hip.h: cge_rccl_unique_id)."""
    buf = C.create_string_buffer(128)
    rc = load_library().cge_rccl_unique_id(buf)
    if rc:
        raise CGEError(rc, "cge_rccl_unique_id failed (is librccl installed and a GPU visible?)")
    return buf.raw


def idx(n, i, j):
    return load_library().cge_idx(n, i, j)


# ---- the reference's exported functions ------------------------------------------------------------------
def landmarks(edges, weights, vweights, clusters, comm, embedding, verbose, land, forced, method, directed,
              ctx: Context | None = None):
    """landmarks(edges, weights, vweights, clusters, comm, embedding, verbose, land, forced, method, directed)
    -> (dii, embed, cluster, landmark_edges, weights, lweight, v_to_l)        (src/landmarks.jl:365-367, :465)"""
    ctx = ctx or default_context()
    verbose and print("Starts landmark generation")
    ctx.set_inputs(edges, weights, vweights, comm, embedding)
    N, _, truncated = ctx.landmarks_run(clusters, land, forced, method, directed)
    if truncated:
        print("Warning: Requested number of clusters larger than unique no. embeddings. Truncating.", file=sys.stderr)
    verbose and print("Landmarks generated")
    verbose and print(f"Using {N} landmarks")
    return ctx.landmarks_fetch()


def _wgcl(directed, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
          init_eweights, init_embed, split, seed, auc_samples, verbose, samples, trace, ctx):
    ctx = ctx or default_context()
    if verbose:  # the reference's own lines, in its order (src/divergence.jl:43-52,75 / :296-305,354)
        e = np.asarray(edges)
        ie = np.asarray(init_edges) if init_edges is not None else np.zeros((0, 2), np.int64)
        print(f"auc_samples: {auc_samples}")
        print(f"Graph has {int(e.max())} vertices and {e.shape[0]} edges")
        if v_to_l is not None and len(v_to_l) > 0 and ie.size:
            print(f"Original graph has {int(ie.max())} vertices and {ie.shape[0]} edges")
        print(f"Graph has {int(np.asarray(comm).max())} communities")
        print(f"Embedding has {np.asarray(embed).shape[1]} dimensions")
    res = ctx.wgcl(edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
                   init_eweights, init_embed, split, seed, auc_samples, verbose, directed, samples)
    sys.stderr.write("." * ctx.last_trace["n_alpha"] + "\n")  # src/divergence.jl:140,255
    return (res, ctx.last_trace) if trace else res


def wGCL(edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges, init_eweights,
         init_embed, split, seed=-1, auc_samples=10000, verbose=False, *, samples=None, trace=False, ctx=None):
    """src/divergence.jl:27-31.  `samples` (optional) = pre-drawn (pos_idx, neg_i, neg_j), each (n_sets, S)."""
    return _wgcl(False, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
                 init_eweights, init_embed, split, seed, auc_samples, verbose, samples, trace, ctx)


def wGCL_directed(edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
                  init_eweights, init_embed, split, seed=-1, auc_samples=10000, verbose=False, *, samples=None,
                  trace=False, ctx=None):
    """src/divergence.jl:282-286."""
    return _wgcl(True, edges, eweights, comm, embed, distances, vweights, init_vweights, v_to_l, init_edges,
                 init_eweights, init_embed, split, seed, auc_samples, verbose, samples, trace, ctx)


def score(edges, eweights, vweights, comm, clusters, embedding, land, forced=4, method="rss", directed=False,
          split=False, seed=-1, auc_samples=10000, ctx=None):
    ctx = ctx or default_context()
    ctx.set_inputs(edges, eweights, vweights, comm, embedding)
    return ctx.score(clusters, land, forced, method, directed, split, seed, auc_samples)


def score_batch(edges, eweights, vweights, comm, clusters, embeddings, land, forced=4, method="rss", directed=False,
                split=False, seed=-1, auc_samples=10000, ctx=None):
    """`score` for several embeddings of one graph: a list of result vectors (Context.score_batch)."""
    ctx = ctx or default_context()
    embeddings = list(embeddings)
    n = int(np.asarray(embeddings[0]).shape[0])
    ctx.set_graph(edges, eweights, n)
    ctx.set_vertex_data(comm, vweights)
    return ctx.score_batch(embeddings, clusters, land, forced, method, directed, split, seed, auc_samples)


def score_tensors(edge_index, embeddings, comm, land, forced=4, method="rss", directed=False, split=False, seed=-1,
                  auc_samples=10000, weights=None, base=-1, ctx=None):
    """The whole call on tensors as held: `edge_index` ((2, m) or (m, 2), int32 / int64, 0- or 1-based), one embedding or a list
    of embeddings ((n, d); float64 / float32 / float16 / bfloat16), `comm` (n community ids) -- numpy arrays or torch tensors,
    host or GPU.  The graph goes in as a view, the vertex weights and the clusters are derived by the library, the embeddings are
    scored by `score_views`.  Returns the result vector (one embedding) or the list of vectors; traces in `ctx.last_traces`."""
    ctx = ctx or default_context()
    one = hasattr(embeddings, "shape") and len(embeddings.shape) == 2
    members = [embeddings] if one else list(embeddings)
    if not members:
        raise ValueError("score_tensors: no embeddings")
    ctx.set_graph_view(edge_index, weights, n=int(members[0].shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    res = ctx.score_views(members, FROM_COMM, land, forced, method, directed, split, seed, auc_samples)
    return res[0] if one else res


def link_predict(edge_index, embedding, comm, land, queries, k, forced=4, method="rss", directed=False, split=False, seed=-1,
                 auc_samples=10000, which="local", exclude_edges=True, weights=None, base=-1, ctx=None):
    """Link prediction on tensors as held, in the manner of `score_tensors`: the graph and the embedding go in as views, the
    model of the best alpha (`which`) is fitted by `Context.link_fit`, and the k most probable candidates of every query vertex
    come back from `Context.link_topk`.  `queries`: 1-based vertex ids (None: every vertex).  Returns (vector, j, p, count);
    the model stays in the context for `link_prob` / further `link_topk` calls."""
    ctx = ctx or default_context()
    ctx.set_graph_view(edge_index, weights, n=int(embedding.shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    ctx.set_embedding_view(embedding)
    vec, _ = ctx.link_fit(FROM_COMM, land, forced, method, directed, split, seed, auc_samples, which)
    if len(vec) < 7:  # a directed star graph: the reference's early return, no model
        return vec, None, None, None
    q = np.arange(1, ctx.n + 1, dtype=np.int64) if queries is None else queries
    return (vec,) + ctx.link_topk(q, k, exclude_edges)


def link_metrics(greater, ties, cand, ks=(1, 10, 50, 100)):
    """The usual link-prediction figures from `Context.link_rank`'s counts (pure numpy, no GPU).  With the realistic rank
    1 + greater + ties / 2 of every pair: {"mrr", "hits@k" for every k of `ks` (the share of pairs of rank <= k), "mean_rank",
    "auc" (the mean of 1 - (greater + ties / 2) / cand over the pairs with cand > 0), "mrr_optimistic" (ranks 1 + greater),
    "mrr_pessimistic" (ranks 1 + greater + ties)}.  A figure over no pairs is NaN."""
    g, t, c = (np.asarray(x, dtype=np.float64).ravel() for x in (greater, ties, cand))
    if not len(g) == len(t) == len(c):
        raise ValueError("link_metrics: greater, ties and cand differ in length")

    def mean(v):
        return float(np.mean(v)) if len(v) else float("nan")

    rank = 1.0 + g + 0.5 * t
    out = {"mrr": mean(1.0 / rank)}
    for k in ks:
        out[f"hits@{int(k)}"] = mean(rank <= k)
    out["mean_rank"] = mean(rank)
    has = c > 0
    out["auc"] = mean(1.0 - (g[has] + 0.5 * t[has]) / c[has])
    out["mrr_optimistic"] = mean(1.0 / (1.0 + g))
    out["mrr_pessimistic"] = mean(1.0 / (1.0 + g + t))
    return out


def link_evaluate(edge_index, embedding, comm, land, test_pairs, forced=4, method="rss", directed=False, split=False, seed=-1,
                  auc_samples=10000, which="local", exclude_edges=True, ks=(1, 10, 50, 100), weights=None, base=-1, ctx=None):
    """Evaluation of the fitted model on held-out pairs, beside `link_predict`: the (training) graph and the embedding go in as
    views, `Context.link_fit` fits the model of the best alpha, `Context.link_rank` ranks `test_pairs` ((P, 2) or (2, P) with
    P != 2; 1-based vertex ids) among the non-neighbours of their source, and `link_metrics` sums up.  Returns (vector, metrics,
    (greater, ties, cand, p)); a directed star graph's early return leaves (vector, None, None)."""
    ctx = ctx or default_context()
    ctx.set_graph_view(edge_index, weights, n=int(embedding.shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    ctx.set_embedding_view(embedding)
    vec, _ = ctx.link_fit(FROM_COMM, land, forced, method, directed, split, seed, auc_samples, which)
    if len(vec) < 7:
        return vec, None, None
    tp = _i64(_host_array(test_pairs))
    if tp.ndim != 2 or 2 not in tp.shape:
        raise ValueError("link_evaluate: test_pairs is (P, 2) or (2, P)")
    if tp.shape[1] != 2:
        tp = tp.T
    counts = ctx.link_rank(tp[:, 0], tp[:, 1], exclude_edges)
    return vec, link_metrics(counts[0], counts[1], counts[2], ks), counts


def _link_auc_quotients(W, L, Tq, n_neg):
    """(1 - L / (W n_neg), (L + Tq / 2) / (W n_neg)) in long double, rounded once each; NaN without non-edges or weight."""
    LD = np.longdouble
    den = LD(W) * LD(int(n_neg))
    if not den > 0:
        return float("nan"), float("nan")
    return float(LD(1) - LD(L) / den), float((LD(L) + LD(Tq) / LD(2)) / den)


def link_auc_from_counts(less, ties, w, n_neg):
    """The two quotients of `Context.link_auc` from per-edge counts (pure numpy in long double, no GPU): for callers who add the
    parts' `less` / `ties` up.  `w`: the edge weights (None: 1 each).  Returns {"local_exact", "auc", "W", "L", "Tq"}; the sums
    are taken in the list's order in long double and rounded once, as the library takes them."""
    LD = np.longdouble
    ls, ts = np.asarray(less).ravel(), np.asarray(ties).ravel()
    ww = np.ones(len(ls)) if w is None else np.asarray(w, dtype=np.float64).ravel()
    if not len(ls) == len(ts) == len(ww):
        raise ValueError("link_auc_from_counts: less, ties and w differ in length")
    W, L, Tq = LD(0), LD(0), LD(0)
    for a, b, c in zip(ww.astype(LD), ls.astype(LD), ts.astype(LD)):  # (np.sum adds pairwise: another order)
        W += a
        L += a * b
        Tq += a * c
    W, L, Tq = float(W), float(L), float(Tq)
    le, auc = _link_auc_quotients(W, L, Tq, n_neg)
    return {"local_exact": le, "auc": auc, "W": W, "L": L, "Tq": Tq}


def link_auc(edge_index, embedding, comm, land, forced=4, method="rss", directed=False, split=False, seed=-1, auc_samples=10000,
             which="local", want_counts=False, want_p=False, weights=None, base=-1, ctx=None):
    """The exact local score and AUC of the fitted model, beside `link_evaluate`: the graph and the embedding go in as views,
    `Context.link_fit` fits the model of the best alpha, `Context.link_auc` counts every non-edge against every edge.  Returns
    (vector, result); a directed star graph's early return leaves (vector, None)."""
    ctx = ctx or default_context()
    ctx.set_graph_view(edge_index, weights, n=int(embedding.shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    ctx.set_embedding_view(embedding)
    vec, _ = ctx.link_fit(FROM_COMM, land, forced, method, directed, split, seed, auc_samples, which)
    if len(vec) < 7:
        return vec, None
    return vec, ctx.link_auc(0, 1, want_counts, want_p)


class LinkMoments:
    """What `Context.link_moments` returns: deg_out, deg_in (n), B, V, C (L, the sweep's bin layout), n_comm, directed."""
    __slots__ = ("deg_out", "deg_in", "B", "V", "C", "n_comm", "directed")

    def __init__(self, deg_out, deg_in, B, V, C_, n_comm, directed):
        self.deg_out, self.deg_in, self.B, self.V, self.C, self.n_comm, self.directed = deg_out, deg_in, B, V, C_, n_comm, directed


def link_bin_pairs(n_comm, directed):
    """The community pair (a, b), 1-based, of every bin of the sweep's layout: cge_idx(C, a, b) order with a <= b when
    undirected (L = C (C + 1) / 2), (a - 1) C + b when directed (L = C C).  Returns (a, b), int64 (L,) each."""
    nc = int(n_comm)
    if directed:
        a, b = np.divmod(np.arange(nc * nc, dtype=np.int64), nc)
        return a + 1, b + 1
    a = np.repeat(np.arange(1, nc + 1, dtype=np.int64), np.arange(nc, 0, -1))
    b = np.concatenate([np.arange(i, nc + 1, dtype=np.int64) for i in range(1, nc + 1)]) if nc else np.zeros(0, np.int64)
    return a, b


def link_bins_table(B, V, C_, n_comm, directed):
    """Per community bin the observed edge mass beside the model's: rows (a, b, observed, expected, sd, z) with observed = C[bin]
    (the sweep's vect_C), expected = B[bin], sd = sqrt(V[bin]) and z = (observed - expected) / sd -- 0 where both the difference
    and sd are 0, +-inf where only sd is.  V is the variance of a draw's edge COUNT, so z means something for an unweighted graph
    only (unit edge weights: the observed mass is a count).  Returns a list of tuples in the bins' order."""
    Bv, Vv, Cv = (np.asarray(x, dtype=np.float64).ravel() for x in (B, V, C_))
    a, b = link_bin_pairs(n_comm, directed)
    if not len(Bv) == len(Vv) == len(Cv) == len(a):
        raise ValueError(f"link_bins_table: B, V, C of {len(Bv)}, {len(Vv)}, {len(Cv)} bins, the layout has {len(a)}")
    sd = np.sqrt(np.maximum(Vv, 0.0))
    diff = Cv - Bv
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0, diff / sd, np.where(diff == 0, 0.0, np.sign(diff) * np.inf))
    return [(int(a[k]), int(b[k]), float(Cv[k]), float(Bv[k]), float(sd[k]), float(z[k])) for k in range(len(a))]


def link_divergence(C_, B, n_comm, directed, split, ctx=None, js=None):
    """The Jensen-Shannon figures of a score's elements 2-4 for the bin vectors (C, B): {"global", "external", "internal"}.
    Without split: global = JS(C, B) over all bins, the other two 0.0; with split: internal over the bins (a, a), external over
    the others, global their mean (src/divergence.jl:235-241, :539-545).  JS is the library's (`Context.js` of ctx or the default
    context); js = a callable (vC, vB, vI, internal) replaces it."""
    Cv, Bv = (np.asarray(x, dtype=np.float64).ravel() for x in (C_, B))
    a, b = link_bin_pairs(n_comm, directed)
    if not len(Cv) == len(Bv) == len(a):
        raise ValueError(f"link_divergence: C, B of {len(Cv)}, {len(Bv)} bins, the layout has {len(a)}")
    if js is None:
        js = (ctx or default_context()).js
    if not split:
        return {"global": float(js(Cv, Bv, None, True)), "external": 0.0, "internal": 0.0}
    vI = (a == b).astype(np.uint8)
    d_int, d_ext = float(js(Cv, Bv, vI, True)), float(js(Cv, Bv, vI, False))
    return {"global": (d_int + d_ext) / 2.0, "external": d_ext, "internal": d_int}


def link_moments(edge_index, embedding, comm, land, forced=4, method="rss", directed=False, split=False, seed=-1, auc_samples=10000,
                 which="global", diag=False, weights=None, base=-1, ctx=None):
    """The moments of the fitted model, beside `link_auc`: the graph and the embedding go in as views, `Context.link_fit` fits
    the model of the best alpha (by default the best divergence's), `Context.link_moments` sums it over every pair.  Returns
    (vector, LinkMoments); a directed star graph's early return leaves (vector, None)."""
    ctx = ctx or default_context()
    ctx.set_graph_view(edge_index, weights, n=int(embedding.shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    ctx.set_embedding_view(embedding)
    vec, _ = ctx.link_fit(FROM_COMM, land, forced, method, directed, split, seed, auc_samples, which)
    if len(vec) < 7:
        return vec, None
    return vec, ctx.link_moments(diag)


def link_clustering_table(tri_exp, wed_exp, tri_obs, wed_obs, summary, comm=None):
    """What `link_clustering` derives from `Context.link_triangles`' arrays: {"tri_exp", "wed_exp", "tri_obs", "wed_obs",
    "c_exp" = tri_exp / wed_exp and "c_obs" = tri_obs / wed_obs per vertex (NaN where there are no wedges), "transitivity_exp" =
    summary[0] / summary[1], "transitivity_obs" = summary[2] / summary[3] (NaN for a zero wedge sum), "triangles_exp" /
    "triangles_obs" = the sums / 3, "summary"}; with comm (n, ids in any base) also "communities" (the distinct ids ascending) and
    "by_community" ((len, 4): per community the sums of tri_obs, wed_obs, tri_exp, wed_exp over its vertices)."""
    te, we = np.asarray(tri_exp, dtype=np.float64), np.asarray(wed_exp, dtype=np.float64)
    to, wo = np.asarray(tri_obs, dtype=np.int64), np.asarray(wed_obs, dtype=np.int64)
    s = [float(x) for x in summary]
    with np.errstate(divide="ignore", invalid="ignore"):
        c_exp = np.where(we > 0, te / we, np.nan)
        c_obs = np.where(wo > 0, to / np.where(wo > 0, wo, 1), np.nan)
    out = {"tri_exp": te, "wed_exp": we, "tri_obs": to, "wed_obs": wo, "c_exp": c_exp, "c_obs": c_obs, "summary": np.array(s),
           "transitivity_exp": s[0] / s[1] if s[1] > 0 else float("nan"),
           "transitivity_obs": s[2] / s[3] if s[3] > 0 else float("nan"), "triangles_exp": s[0] / 3.0, "triangles_obs": s[2] / 3.0}
    if comm is not None:
        ids, inv = np.unique(np.asarray(comm).ravel(), return_inverse=True)
        if len(inv) != len(te):
            raise ValueError(f"link_clustering_table: comm has {len(inv)} entries, the arrays {len(te)}")
        out["communities"] = ids
        out["by_community"] = np.stack([np.bincount(inv, weights=x.astype(np.float64), minlength=len(ids))
                                        for x in (to, wo, te, we)], axis=1)
    return out


def link_clustering(edge_index, embedding, comm, land, forced=4, method="rss", split=False, seed=-1, auc_samples=10000,
                    which="local", weights=None, base=-1, ctx=None):
    """How much of the graph's clustering the fitted model explains, beside `link_moments`: the graph and the embedding go in as
    views, `Context.link_fit` fits the (undirected) model of the best alpha, `Context.link_triangles` gives expected and observed
    triangles and wedges per vertex.  Returns (vector, `link_clustering_table`'s dict with the per-community sums)."""
    ctx = ctx or default_context()
    ctx.set_graph_view(edge_index, weights, n=int(embedding.shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    ctx.set_embedding_view(embedding)
    vec, _ = ctx.link_fit(FROM_COMM, land, forced, method, False, split, seed, auc_samples, which)
    if len(vec) < 7:
        return vec, None
    return vec, link_clustering_table(*ctx.link_triangles(), comm=_host_array(comm))


def link_sample(edge_index, embedding, comm, land, forced=4, method="rss", directed=False, split=False, seed=-1, auc_samples=10000,
                which="local", sample_seed=0, samples=1, want_p=False, weights=None, base=-1, ctx=None):
    """Random graphs from the fitted model, beside `link_predict`: the graph and the embedding go in as views, `Context.link_fit`
    fits the model of the best alpha once, and `samples` draws follow on the streams 0 .. samples - 1 of `sample_seed`
    (`Context.link_sample`).  Returns (vector, [(i, j, p or None, n_edges), ...]); a directed star graph's early return leaves
    (vector, None)."""
    ctx = ctx or default_context()
    ctx.set_graph_view(edge_index, weights, n=int(embedding.shape[0]), base=base)
    ctx.set_vertex_view(comm, None, base=base)
    ctx.set_embedding_view(embedding)
    vec, _ = ctx.link_fit(FROM_COMM, land, forced, method, directed, split, seed, auc_samples, which)
    if len(vec) < 7:
        return vec, None
    return vec, [ctx.link_sample(sample_seed, r, None, want_p) for r in range(int(samples))]


def draw_samples(ctx, seed, S, directed=False, n_sets=1):
    sets = [ctx.draw_samples(seed, S, directed, t) for t in range(n_sets)]
    return tuple(np.stack([s[k] for s in sets]) for k in range(3))
