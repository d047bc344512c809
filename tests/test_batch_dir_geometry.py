"""CPU tests of the directed batch's host arithmetic (no GPU): the geometry of the directed persistent fit as the library
computes it (hook cge_fit_dir_geometry_test -- flow_geometry, the one function every persistent fit's launch asks) against the
formulas restated here, and the launch groups a directed batch forms on it (cge_batch_pack_dir_test, batch_group_closes).  This
pins "a member of a shared launch runs the geometry of its own launch"."""
import os

import pytest

from conftest import ROOT

CUS = [256, 304, 64]


def _geometry(N, cus):
    """fit_flow_dir_kernel's launch shape: one 64 x 64 upper tile per wave, NW = 4 waves per workgroup while 4 * cus waves cover
    the triangle, else 8; one workgroup per NW tiles and at least one per quarter block (16 rows) where the CUs allow."""
    Nt = (N + 63) // 64
    NT = Nt * (Nt + 1) // 2
    if Nt > 64:
        return None
    NW = 4 if NT <= 4 * cus else 8
    G = min(cus, max((NT + NW - 1) // NW, 4 * Nt))
    if NT > NW * G or 4 * Nt > 2 * G:
        return None
    return G, NW, 1 if 4 * Nt <= G else 2


def _member(N, cus):
    g = _geometry(N, cus)
    return g if g and N >= 256 and g[2] == 1 and g[0] <= cus // 2 else None


def _sizes():
    Ns = {1, 2, 255, 256, 257, 400, 1000, 1984, 1985, 4032, 4033, 4096, 4097, 5000}
    for k in range(1, 66):
        Ns.update((64 * k - 1, 64 * k, 64 * k + 1))
    return sorted(Ns)


@pytest.mark.parametrize("cus", CUS)
def test_geometry_hook_equals_the_formulas(cus):
    from cge.jl_amd import api

    seen = set()
    for N in _sizes():
        got, exp = api.fit_dir_geometry_test(N, cus), _geometry(N, cus)
        assert got == exp, (N, cus, got, exp)
        seen.add(None if exp is None else (exp[1], exp[2]))
    assert None in seen and {nw for nw, _ in seen - {None}} == {4, 8}  # the sizes reach both wave counts and the refusal
    if cus == 64:
        assert {(4, 1), (4, 2), (8, 2)} <= seen  # a small chip: two quarter blocks per workgroup
    else:
        assert seen == {None, (4, 1), (8, 1)}  # (capped by the CUs only beyond Nt = 64, which the form declines)


def test_the_sizes_people_compare_embeddings_at():
    from cge.jl_amd import api

    assert api.fit_dir_geometry_test(400, 256) == (28, 4, 1)  # 7 x 7 tiles, 28 upper tiles: max(7, 28)
    assert api.fit_dir_geometry_test(1000, 256) == (64, 4, 1)
    assert api.fit_dir_geometry_test(1300, 256) == (84, 4, 1)
    assert _member(255, 256) is None and _member(256, 256) == (16, 4, 1)
    assert _member(1984, 256) == (124, 4, 1) and _member(1985, 256) is None  # G = 132 > 128: more than half the chip


@pytest.mark.parametrize("cus", CUS)
def test_launch_groups_close_by_workgroups_wave_count_and_sixteen(cus):
    from cge.jl_amd import api

    Ns = [400] * 20 + [100, 1000, 256, 300, 5000, 1000, 1984, 700] + [256] * 40
    n_groups, got = api.batch_pack_dir_test(Ns, cus)
    exp, g_sum, g_nw, g_size, groups = [], 0, 0, 0, 0
    for N in Ns:
        m = _member(N, cus)
        if m is None:
            exp.append(-1)
            continue
        if g_size == 0 or g_sum + m[0] > cus or m[1] != g_nw or g_size >= 16:
            groups, g_sum, g_size = groups + 1, 0, 0
        g_sum, g_nw, g_size = g_sum + m[0], m[1], g_size + 1
        exp.append(groups - 1)
    assert got.tolist() == exp and n_groups == groups
    if cus == 256:
        assert exp[:20] == [0] * 9 + [1] * 9 + [2] * 2  # 9 x 28 = 252 <= 256 < 10 x 28
        assert exp[20] == -1 and exp[24] == -1  # fewer than 256 landmarks; beyond the register file
        assert max(exp.count(g) for g in set(exp) if g >= 0) == 16  # 16 x 16 workgroups fit: the member limit closes the group


def test_hooks_are_declared_and_reject_null_outputs():
    import ctypes as C

    from cge.jl_amd import api

    hdr = open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    assert "int cge_fit_dir_geometry_test(" in hdr and "int cge_batch_pack_dir_test(" in hdr
    L = api.load_library()
    ap = C.c_int()
    assert L.cge_fit_dir_geometry_test(C.c_int64(400), 256, C.byref(ap), None, None, None) == -7
