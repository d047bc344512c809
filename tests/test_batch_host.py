"""CPU tests of cge_score_batch's host side: the entry point is declared and exported, and the packer of its launch groups
(the members' fused fits side by side in one launch) keeps the members' order and the chip's CU count.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT


def _lib():
    from cge.jl_amd import api

    L = api.load_library()
    L.cge_batch_pack_test.restype = C.c_int
    L.cge_batch_pack_test.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    return L


def _pack(Ns, cus=256):
    N = np.ascontiguousarray(Ns, dtype=np.int64)
    out = np.full(len(N), -7, dtype=np.int32)
    n_groups = _lib().cge_batch_pack_test(N.ctypes.data, len(N), cus, out.ctypes.data)
    assert n_groups >= 0
    return n_groups, out.tolist()


def test_score_batch_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    assert re.search(r"int cge_score_batch\(cge_ctx \*ctx, const cge_score_args \*args, const cge_embedding_batch \*batch,", hdr)
    assert "} cge_embedding_batch;" in hdr
    assert "#define CGE_ABI_VERSION 1" in hdr  # an addition: the ABI version stays
    L = _lib()
    assert hasattr(L, "cge_score_batch")
    assert L.cge_abi_version() == 1


def test_score_batch_rejects_bad_arguments_before_any_work():
    from cge.jl_amd import api

    L = _lib()
    # a NULL context / NULL batch fail at the boundary without touching a device
    a = api.ScoreArgs()
    out = np.zeros(7)
    olen = (C.c_int * 1)(5)
    assert L.cge_score_batch(None, C.byref(a), None, out.ctypes.data, olen, None) == -7
    b = api.EmbeddingBatch()
    b.K = 0
    assert L.cge_score_batch(None, C.byref(a), C.byref(b), out.ctypes.data, olen, None) == -7


def test_pack_twenty_members_of_400_landmarks_in_groups_of_nine():
    # N = 400: 7 x 7 tiles, 28 upper tiles, G = max(28 / 4, 4 * 7) = 28 workgroups; 9 x 28 = 252 <= 256 < 10 x 28
    n_groups, g = _pack([400] * 20)
    assert n_groups == 3
    assert g == [0] * 9 + [1] * 9 + [2] * 2


def test_pack_a_member_that_fills_the_chip_is_a_group_of_one():
    n_groups, g = _pack([4000] * 3)
    assert n_groups == 3 and g == [0, 1, 2]


def test_pack_keeps_the_order_and_leaves_out_what_is_not_batched():
    # 100 landmarks: no fused fit (scored on its own, -1); 4000 between two small members closes both neighbouring groups
    n_groups, g = _pack([400, 400, 100, 4000, 400, 1000])
    assert g[2] == -1
    assert g[0] == g[1] == 0 and g[3] == 1 and g[4] == 2
    assert n_groups == 3 and g[5] == 2  # 28 + 64 workgroups, the same four waves per workgroup
    assert g == sorted(g[:2]) + [-1] + sorted(g[3:])  # groups in member order


def test_pack_respects_the_cu_count_it_is_given():
    # the same members on a chip of 64 CUs: two of 28 per group
    n_groups, g = _pack([400] * 5, cus=64)
    assert n_groups == 3 and g == [0, 0, 1, 1, 2]
    # every group fits: the sum of its members' workgroups is at most the CU count (G as fit_flow_kernel sizes its grid)
    def G_of(N, cus=256):
        Nt = -(-N // 64)
        NT = Nt * (Nt + 1) // 2
        NW = 4 if NT <= 4 * cus else 8
        return min(cus, max(-(-NT // NW), 4 * Nt))

    Ns = [256, 300, 400, 700, 1000, 1500, 2000] * 3
    n_groups, g = _pack(Ns, cus=256)
    assert g == sorted(g) and min(g) == 0 and n_groups == max(g) + 1
    for q in range(n_groups):
        assert sum(G_of(n) for n, gg in zip(Ns, g) if gg == q) <= 256


def test_pack_at_most_sixteen_members_per_group():
    n_groups, g = _pack([256] * 20)  # G = 16 each: sixteen fill 256 CUs
    assert g == [0] * 16 + [1] * 4 and n_groups == 2


def test_compare_script_splits_its_embeddings():
    import sys

    sys.path.insert(0, ROOT)
    try:
        import cge_compare
    finally:
        sys.path.pop(0)
    argv, files = cge_compare.split_embeddings(["-g", "g.txt", "-e", "a.emb", "-l", "400", "-e", "b.emb", "--seed", "1"])
    assert files == ["a.emb", "b.emb"]
    assert argv == ["-g", "g.txt", "-l", "400", "--seed", "1", "-e", "a.emb"]
