"""CPU tests of the persistent fits' host arithmetic (no GPU): the ONE launch geometry every path takes (flow_geometry, through the
hook cge_fit_dir_geometry_test), the members a batch groups on it (cge_batch_pack_test, cge_batch_pack_dir_test) and the ONE
layout of a problem's hand-off slots (flow_slots, through cge_fit_slots_test), each against the formulas restated here, for every
N a fit can be asked for."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

CUS = [64, 80, 256, 304]
N_MAX = 4300


def _geometry(N, cus):
    """(G, NW, NSB), or the reason of the refusal.  One 64 x 64 upper tile per wave, NW = 4 waves per workgroup while 4 * cus
    waves cover the triangle, else 8; one workgroup per NW tiles and at least one per quarter block (16 rows) where the CUs allow;
    NSB = quarter blocks a workgroup may have to reduce."""
    if N <= 0 or cus <= 0:
        return "empty"
    Nt = (N + 63) // 64
    NT = Nt * (Nt + 1) // 2
    if Nt > 64:
        return "blocks"  # a reducer adds up to 64 partial vectors
    NW = 4 if NT <= 4 * cus else 8
    G = min(cus, max((NT + NW - 1) // NW, 4 * Nt))
    if NT > NW * G:
        return "tiles"  # more tiles than waves
    if 4 * Nt > 2 * G:
        return "quarters"  # more than two quarter blocks per workgroup
    return G, NW, 1 if 4 * Nt <= G else 2


def _member(N, cus, directed):
    g = _geometry(N, cus)
    if isinstance(g, str) or N < 256 or g[2] != 1 or (directed and g[0] > cus // 2):
        return None
    return g


def _pack(name, Ns, cus):
    from cge.jl_amd import api

    fn = getattr(api.load_library(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    N = np.ascontiguousarray(Ns, dtype=np.int64)
    out = np.full(len(N), -2, np.int32)
    n = fn(N.ctypes.data, len(N), int(cus), out.ctypes.data)
    assert n >= 0
    return n, out.tolist()


@pytest.mark.parametrize("cus", CUS)
def test_geometry_of_every_size(cus):
    from cge.jl_amd import api

    seen = set()
    for N in range(1, N_MAX + 1):
        got, exp = api.fit_dir_geometry_test(N, cus), _geometry(N, cus)
        assert got == (None if isinstance(exp, str) else exp), (N, cus, got, exp)
        seen.add(exp if isinstance(exp, str) else exp[1:])
    assert {(4, 1), "blocks"} <= seen and any(s[0] == 8 for s in seen if not isinstance(s, str))
    if cus == 64:
        assert {(4, 2), (8, 2), "tiles"} <= seen  # a small chip: two quarter blocks per workgroup, then too few waves
    if cus == 256:
        assert {(8, 1), "tiles"} <= seen  # Nt = 64: 2080 tiles on 2048 waves
    for N in (0, -1):
        assert api.fit_dir_geometry_test(N, cus) is None
    assert api.fit_dir_geometry_test(400, 0) is None and api.fit_dir_geometry_test(400, -4) is None


def test_geometry_refuses_a_third_quarter_block():
    from cge.jl_amd import api

    assert _geometry(300, 8) == "quarters" and api.fit_dir_geometry_test(300, 8) is None  # 5 x 5 blocks: 20 quarters on 8 CUs
    assert _geometry(256, 8) == (8, 4, 2) and api.fit_dir_geometry_test(256, 8) == (8, 4, 2)


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("cus", CUS)
def test_batch_members_of_every_size(cus, directed):
    """The packers group exactly the members of >= 256 landmarks with one quarter block per workgroup -- directed ones also on at
    most half the chip -- and close a group when the next member's workgroups would exceed the CUs, its waves per workgroup differ
    or the group holds 16 members."""
    Ns = list(range(1, N_MAX + 1))
    n_groups, got = _pack("cge_batch_pack_dir_test" if directed else "cge_batch_pack_test", Ns, cus)
    exp, g_sum, g_nw, g_size, groups = [], 0, 0, 0, 0
    for N in Ns:
        m = _member(N, cus, directed)
        if m is None:
            exp.append(-1)
            continue
        if g_size == 0 or g_sum + m[0] > cus or m[1] != g_nw or g_size >= 16:
            groups, g_sum, g_size = groups + 1, 0, 0
        g_sum, g_nw, g_size = g_sum + m[0], m[1], g_size + 1
        exp.append(groups - 1)
    assert got == exp and n_groups == groups
    batched = [N for N, g in zip(Ns, got) if g >= 0]
    assert batched and batched[0] == 256
    assert all(not isinstance(_geometry(N, cus), str) and _geometry(N, cus)[2] == 1 for N in batched)
    if directed:
        assert max(_geometry(N, cus)[0] for N in batched) <= cus // 2
    else:  # (the undirected packer keeps members beyond half the chip: a group of one)
        assert max(_geometry(N, cus)[0] for N in batched) > cus // 2


def _slots(Nt, directed):
    Tld = 64 * Nt
    ring = 32  # 32 doubles of sync words first
    fq = ring + (8 if directed else 4) * Tld  # the T ring: 4 x T, directed 4 x (Tin, Tout)
    P = fq + 12 * Nt  # f: 3 x 4 Nt
    return {"sync": 0, "ring": ring, "fq": fq, "P": P, "doubles": P + (4 if directed else 2) * Nt * Nt * 64}


@pytest.mark.parametrize("directed", [False, True])
def test_slot_layout_of_every_block_count(directed):
    from cge.jl_amd import api

    prev = None
    for Nt in range(1, 65):
        s = api.fit_slots_test(64 * Nt, directed)
        assert s == _slots(Nt, directed) == api.fit_slots_test(64 * Nt - 63, directed), (Nt, s)
        assert s["doubles"] % 2 == 0  # armed in 16-byte units
        Tld = 64 * Nt
        sizes = [32, (8 if directed else 4) * Tld, 12 * Nt, (4 if directed else 2) * Nt * Nt * 64]
        starts = [s["sync"], s["ring"], s["fq"], s["P"], s["doubles"]]
        assert starts[0] == 0 and [b - a for a, b in zip(starts, starts[1:])] == sizes  # no gap, no overlap
        if prev:  # two problems back to back: the second starts at the first's total, behind the first's last slot
            second = {k: prev["doubles"] + v for k, v in s.items()}
            assert second["sync"] == prev["doubles"] == prev["P"] + (prev["doubles"] - prev["P"])
            assert second["sync"] % 2 == 0 and second["doubles"] == prev["doubles"] + s["doubles"]
        prev = s


def test_slots_hook_is_declared_and_checks_its_arguments():
    from cge.jl_amd import api

    hdr = open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    assert "int cge_fit_slots_test(int64_t N, int directed, int64_t out[5]);" in hdr
    L = api.load_library()
    out = (C.c_int64 * 5)()
    assert L.cge_fit_slots_test(C.c_int64(400), 0, None) == -7
    for N in (0, -1, 4097):
        assert L.cge_fit_slots_test(C.c_int64(N), 1, out) == -7
