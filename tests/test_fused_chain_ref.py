"""tests/fused_chain_ref.py pinned on the CPU: the references tests/test_gpu_fused_chain.py holds the fused epilogue to agree
with each other and with hand-made cases, the shapes have the piece counts they are chosen for, the tally inputs leave no
comparison within reach of a one-ulp difference of `pow`, and the geometry formulas give the sizes the GPU test relies on."""
import numpy as np
import pytest

import fused_chain_ref as fc

LD = fc.LD

FUSED = ["256x2", "257x5", "321x3", "513x8", "700x17", "640x10e", "pieces32"]


def _problem(name, seed=3):
    comm, C = fc.shuffled_comm(name, seed)
    N = comm.size
    rng = np.random.default_rng(seed + 1)
    GD = rng.random((N, N))
    GD = np.triu(GD) + np.triu(GD, 1).T
    T = rng.uniform(0.1, 3.0, N)
    return comm, C, GD, T


def test_layout_by_hand():
    """Six vertices would be one block; 70 give two: ids 1..3 of sizes 3, 0 (empty), 67 in a shuffled order."""
    comm = np.array([3] * 30 + [1] + [3] * 20 + [1, 1] + [3] * 17)
    lay = fc.layout(comm, 3)
    assert lay["order"][:3].tolist() == [30, 51, 52] and lay["order"][3] == 0 and lay["order"][-1] == 69
    assert lay["Nt"] == 2 and lay["fc"].tolist() == [0, 2] and lay["ns"].tolist() == [3, 1]
    assert lay["base"].tolist() == [0, 9, 12, 12] and lay["bt_total"] == 13
    # block 0: 8 chunk starts + the change at vertex 3; block 1: 6 live vertices, then the tail (a run of its own at q = 6)
    assert lay["pieces"].tolist() == [9, 9]


@pytest.mark.parametrize("name", FUSED + ["pieces33", "1100x600", "1985x40", "2817x50"])
def test_every_shape_has_the_piece_count_it_is_chosen_for(name):
    comm, C = fc.shuffled_comm(name, 5)
    s = fc.sizes(name)
    assert comm.size == sum(s) and C == len(s) and np.array_equal(np.bincount(comm - 1, minlength=C), s)
    lay = fc.layout(comm, C)
    top = int(lay["pieces"].max())
    spans = int(lay["ns"].max())
    if name == "pieces32":
        assert lay["pieces"][0] == fc.NP == top
    elif name == "pieces33":
        assert lay["pieces"][0] == fc.NP + 1 and spans <= 64
    elif name == "1100x600":
        assert top > fc.NP and spans <= 64  # the tiles take it, the fused form declines
    else:
        assert top <= fc.NP and spans <= 64
    if name in ("1985x40", "2817x50"):
        assert s.count(1) >= 2 and max(s) <= 120 and min(s) >= 1
    if name == "257x5":
        assert lay["Nt"] == 5 and lay["ns"][-1] == 1 and lay["pieces"][-1] == 9  # one vertex, then the tail as one more run
    if name == "640x10e":
        assert 0 in s and int(lay["ns"].sum()) > sum(len(np.unique(lay["comm_new"][b:b + 64])) for b in range(0, 640, 64))
    if name == "513x8":
        assert lay["ns"][-1] == 1 and lay["comm_new"][-1] == 7


@pytest.mark.parametrize("name", ["256x2", "257x5", "321x3", "640x10e", "pieces32"])
def test_the_bins_are_the_sum_of_the_partials(name):
    comm, C, GD, T = _problem(name)
    lay = fc.layout(comm, C)
    val, cnt = fc.partials(GD, T, lay)
    ref, nk = fc.vect_b(GD, T, comm, C)
    assert np.array_equal(fc.fold(cnt, lay), nk) and nk.sum() == comm.size * (comm.size + 1) // 2
    got = fc.fold(val, lay)
    # long double rounding: every bin was added twice in different orders
    assert np.all(np.abs(got - ref) <= (LD(nk) + 2) * np.finfo(LD).eps * ref)
    assert np.all(got[nk == 0] == 0) and np.all(val[cnt == 0] == 0)
    # a partial is a brute-force sum over its rectangle (a few, the diagonal tile among them)
    o, cn, Nt = lay["order"], lay["comm_new"], lay["Nt"]
    for I, J in ((0, 0), (0, Nt - 1), (Nt - 1, Nt - 1)):
        for a in np.unique(cn[64 * I:64 * I + 64])[:2]:
            for b in np.unique(cn[64 * J:64 * J + 64])[-2:]:
                s, k = LD(0), 0
                for i in range(64 * I, min(comm.size, 64 * I + 64)):
                    for j in range(64 * J, min(comm.size, 64 * J + 64)):
                        if cn[i] == a and cn[j] == b and j >= i:
                            s += (LD(T[o[i]]) * LD(T[o[j]])) * LD(GD[o[i], o[j]])
                            k += 1
                pos = lay["base"][I * Nt + J] + (a - lay["fc"][I]) * lay["ns"][J] + (b - lay["fc"][J])
                assert cnt[pos] == k and abs(val[pos] - s) <= (k + 2) * np.finfo(LD).eps * s


def test_tallies_by_hand_and_the_block_of_a_sample():
    T = np.array([1.0, 2.0, 4.0])
    S = 64 * 256 + 3
    aidx = np.zeros((4, S), np.int32)
    aidx[1] = 1  # pos = T0 T1 ppos = 2 ppos; neg = T0 T0 pneg = pneg
    afac = np.ones((8, S))
    ppos, pneg = np.full(S, 0.5), np.full(S, 0.75)
    pneg[[0, 255, 256, S - 1]] = 1.5  # neg wins there
    wts = np.full(S, 0.25)
    aden = np.arange(64.0)
    part = fc.tallies(T, aidx, afac, aden, wts, ppos, pneg)
    assert np.array_equal(part[:, 1], aden)
    exp = np.full(64, 64.0)  # 256 samples of 0.25
    exp[0] += 3 * 0.25 - 3 * 0.25  # block 0 also takes samples 16384 .. 16386; samples 0, 255 and 16386 lose
    exp[1] -= 0.25
    assert np.array_equal(part[:, 0], exp)
    assert fc.min_tally_gap(T, aidx, afac, ppos, pneg) == pytest.approx(0.25)  # the smaller of (1 - 0.75) / 1 and (1.5 - 1) / 1.5


@pytest.mark.parametrize("S", [1, 255, 256, 257, 16389])
@pytest.mark.parametrize("N", [257, 700, 1985])
def test_no_tally_comparison_is_within_reach_of_one_ulp_of_pow(N, S):
    """The GPU test takes T from the device and the powers from the device's own `pow`; here the gap is checked with numpy's pow
    and a T of the fit's typical spread: a relative gap above 1e-6 is 10^9 ulps away from a turned comparison."""
    t = fc.tally_inputs(N, S, 1000 * N + S)
    assert t["aidx"].min() >= 0 and t["aidx"].max() < N and t["afac"].min() >= 0.5 and t["afac"].max() <= 2.0
    assert np.all(t["wts"] * 4 == np.round(t["wts"] * 4)) and t["wts"].min() >= 0.25 and t["wts"].max() <= 2.0
    assert t["wts"].sum() * 4 < 2.0 ** 52  # multiples of 1/4 well inside the mantissa: every sum exact in any order
    T = np.exp(0.5 * np.random.default_rng(N).normal(size=N))
    for alpha in (0.25, 3.0, 10.0):
        gap = fc.min_tally_gap(T, t["aidx"], t["afac"], (1.0 - t["dpos"]) ** alpha, (1.0 - t["dneg"]) ** alpha)
        assert gap > 1e-6, (N, S, alpha, gap)


def test_geometry_on_256_cus():
    g = fc.geometry(1985, 256)
    assert g["G"] == 132 > 4 * 32 and g["Nt"] == 32 and g["NW"] == 4 and g["NSB"] == 1
    assert fc.geometry(1984, 256)["G"] == 4 * 31
    assert fc.geometry(2816, 256)["NW"] == 4 and fc.geometry(2817, 256)["NW"] == 8 and fc.geometry(2817, 256)["NSB"] == 1
    assert fc.geometry(256, 256) == {"Nt": 4, "NT": 10, "G": 16, "NW": 4, "NSB": 1}
    assert fc.geometry(700, 256)["G"] == 44
    assert fc.geometry(4033, 256) is None and fc.geometry(4097, 256) is None


def test_the_hook_is_declared_and_refuses_a_null_context():
    """cge_fused_chain_test is among the declared symbols, the Python structure has the header's size, and a null context or
    null problems are CGE_E_ARG before anything touches a device."""
    import ctypes as C

    from cge.jl_amd import api

    lib = api.load_library()
    assert hasattr(lib, "cge_fused_chain_test")
    p = api.FusedChainProblem()
    assert C.sizeof(p) == 30 * 8  # cge_fused_chain_problem: 22 pointers, 6 int64, alpha, two pairs of 4-byte fields
    p.iters = -5
    assert lib.cge_fused_chain_test(None, C.byref(p), 1, 0, C.c_double(0.25), C.c_double(0.001)) == -7
    assert lib.cge_fused_chain_test(None, None, 1, 0, C.c_double(0.25), C.c_double(0.001)) == -7
    assert p.iters == -5
