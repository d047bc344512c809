"""CPU tests of tests/ecg_ref.py, the numpy restatement of `cge_ecg` (the mixer, the ranks, the members, the 2-core, the weights,
the final hierarchy), and of what the feature has outside the device: the header, the exported symbols, the refusals at the
boundary, the command-line flags.  The GPU tests (test_gpu_ecg.py) then hold the device to the restatement."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import ecg_ref
import louvain_graphs as lg
from conftest import GOLDEN, ROOT
from louvain_levels_ref import levels
from louvain_ref import sync_level1


def test_mixer_known_answers():
    assert ecg_ref.mix(0) == 0xE220A8397B1DCDAF
    assert ecg_ref.mix(1) == 0x910A2DEC89025CC1
    assert ecg_ref.mix(2**64 - 1) == 0xE4D971771B652C20
    x = np.array([0, 1, 2**64 - 1], dtype=np.uint64)
    assert [int(v) for v in ecg_ref._mix_np(x)] == [ecg_ref.mix(int(v)) for v in x]  # the array form is the scalar form


def test_rank_known_answers_and_ranks_are_permutations():
    assert ecg_ref.ranks(42, 0, 8).tolist() == [3, 5, 1, 7, 2, 6, 4, 0]
    assert ecg_ref.ranks(42, 1, 8).tolist() == [1, 0, 5, 4, 7, 6, 2, 3]
    assert ecg_ref.ranks(-1, 3, 5).tolist() == [2, 4, 3, 0, 1]  # the seed's two's-complement bit pattern
    for seed, r, n in ((0, 0, 1), (7, 5, 2), (-3, 63, 1000), (2**63 - 1, 9, 4097)):
        assert np.array_equal(np.sort(ecg_ref.ranks(seed, r, n)), np.arange(n))
    assert not np.array_equal(ecg_ref.ranks(1, 0, 100), ecg_ref.ranks(1, 1, 100))


def test_a_member_is_the_pass_on_the_relabelled_list_read_back():
    e, n = lg.random_multigraph(257, seed=2)
    res = ecg_ref.ecg(e, None, n, 4, 0.25, 9)
    for r in range(4):
        rank = ecg_ref.ranks(9, r, n)
        relabelled = np.stack([rank[e[:, 0]], rank[e[:, 1]]], axis=1)
        comm, nc, q, rounds = sync_level1(relabelled, None, n)
        assert np.array_equal(res["members"][r], comm[rank])
        assert (res["member_nc"][r], res["member_q"][r], res["member_rounds"][r]) == (nc, q, rounds)
    assert len({m.tobytes() for m in res["members"]}) >= 2


def test_one_member_under_its_own_names_is_the_plain_pass():
    for e, n in (lg.random_multigraph(300, seed=1), lg.clique_chain(30, 5, ring=True), lg.star(20)):
        res = ecg_ref.ecg(e, None, n, 1, 0.125, 0, rank_of=lambda r: np.arange(n))
        comm, nc, q, rounds = sync_level1(e, None, n)
        assert np.array_equal(res["members"][0], comm)
        assert (res["member_nc"][0], res["member_q"][0], res["member_rounds"][0]) == (nc, q, rounds)


def test_two_core():
    assert ecg_ref.two_core(*lg.path(257))[0].sum() == 0 and ecg_ref.two_core(*lg.path(257))[1] == 129
    assert ecg_ref.two_core(*lg.star(65))[0].sum() == 0
    core, rounds = ecg_ref.two_core(*lg.cycle(9))
    assert core.all() and rounds == 0
    e = np.concatenate([lg.cycle(9)[0], [[0, 9], [9, 10], [10, 11]]])  # a cycle with a tail
    core, rounds = ecg_ref.two_core(e, 12)
    assert core.tolist() == [True] * 9 + [False] * 3 and rounds == 3
    # repeated edges are separate entries, self loops are none
    assert ecg_ref.two_core(np.array([[0, 1], [1, 0]]), 2)[0].all()
    assert not ecg_ref.two_core(np.array([[0, 1], [1, 1], [1, 1]]), 2)[0].any()


def test_weights_lie_between_the_floor_and_one_and_equal_the_floor_off_the_core():
    e, n = lg.random_multigraph(257, seed=2)
    res = ecg_ref.ecg(e, None, n, 8, 0.125, 3)
    w, core = res["weights"], res["core"]
    assert w.min() >= 0.125 and w.max() <= 1.0 and 0 < core.sum() < n
    off = ~(core[e[:, 0]] & core[e[:, 1]])
    assert off.any() and np.all(w[off] == 0.125)
    loops = (e[:, 0] == e[:, 1]) & core[e[:, 0]]
    assert loops.any() and np.all(w[loops] == 1.0)  # a self loop in the core is co-clustered by every member
    assert np.all(w * 64 == np.floor(w * 64))  # K = 8, w_min = 1/8: multiples of 1/64


def test_ring_of_sixteen_five_cliques_gives_the_cliques():
    e, n = lg.clique_chain(16, 5, ring=True)
    res = ecg_ref.ecg(e, None, n, 16, 1.0 / 16, 42)
    assert res["n_comm"] == 16 and np.array_equal(res["comm"], lg.clique_labels(16, 5))
    assert res["q"] == pytest.approx(160.0 / 176.0 - 1.0 / 16.0, abs=1e-15)  # 160 of 176 edges inside, 16 equal shares of the degree


@pytest.mark.parametrize("m,C,xi,level1,last,ecg", [(15000, 30, 0.2, (0.944, 64), (0.964, 18), (0.975, 32)),
                                                    (15000, 30, 0.45, (0.685, 181), (0.696, 18), (0.711, 30)),
                                                    (12000, 60, 0.5, (0.397, 512), (0.417, 19), (0.543, 38))])
def test_planted_communities_are_found_better_than_by_any_one_level(m, C, xi, level1, last, ecg):
    """A statement about the definition's meaning, checked on the restatement: K = 16, w_min = 1/16, seed 42.  (ARI against the
    planted communities, communities found) for level 1, the last level and ECG; ECG is at least as good as the last level."""
    from cge.jl_amd import synth

    g = synth.abcd_like(3000, m, C, 4, seed=5, xi=xi)
    e, truth, n = np.asarray(g["edges"]) - 1, g["comm"][:, 0], 3000
    lv = levels(e, None, n)
    res = ecg_ref.ecg(e, None, n, 16, 1.0 / 16, 42)
    got = [(round(ecg_ref.ari(c, truth), 3), nc) for c, nc in ((lv[0][0], lv[0][1]), (lv[-1][0], lv[-1][1]), (res["comm"], res["n_comm"]))]
    print(got)
    assert got == [level1, last, ecg]
    assert ecg_ref.ari(res["comm"], truth) >= ecg_ref.ari(lv[-1][0], truth)
    assert len({x.tobytes() for x in res["members"]}) == 16


def test_ecg_is_declared_and_exported():
    from cge.jl_amd import api

    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    assert "typedef struct { int64_t members; double w_min; int64_t seed; int64_t final_level; } cge_ecg_args;" in hdr
    assert re.search(r"int cge_ecg\(cge_ctx \*ctx, const cge_ecg_args \*args, int64_t \*comm_out", hdr)
    assert "#define CGE_ABI_VERSION 1" in hdr  # an addition: the ABI version stays
    assert "int cge_ecg_members_test(void *ctx," in open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    L = api.load_library()
    assert hasattr(L, "cge_ecg") and hasattr(L, "cge_ecg_members_test") and L.cge_abi_version() == 1
    assert C.sizeof(api.EcgArgs) == 32


def test_ecg_refuses_null_arguments_at_the_boundary():
    from cge.jl_amd import api

    L = api.load_library()
    a = api.EcgArgs(16, 0.05, 0, -1)
    out, nc, q = np.zeros(4, dtype=np.int64), C.c_int64(), C.c_double()
    assert L.cge_ecg(None, C.byref(a), out.ctypes.data, C.byref(nc), C.byref(q), None, None) == -7
    assert L.cge_ecg_members_test(None, C.c_int64(4), C.c_int64(0), None, None, None, None, None) == -7


def _files(tmp_path):
    src = os.path.join(GOLDEN, "test115")
    for f in ("test.edgelist", "test1col.ecg", "test_n2v.embedding"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    return [str(tmp_path / f) for f in ("test.edgelist", "test1col.ecg", "test_n2v.embedding")]


def test_with_c_the_ecg_flags_are_not_consulted(tmp_path):
    import cge.jl_amd as cg

    g, c, e = _files(tmp_path)
    plain = cg.parseargs(["-g", g, "-c", c, "-e", e, "-l", "20"], exit_on_error=False)
    for extra in (["--ecg"], ["--ecg", "8"], ["--ecg", "99", "--ecg-wmin", "7"], ["--ecg", "--louvain-level", "2"]):
        a = cg.parseargs(["-g", g, "-c", c, "-e", e, "-l", "20"] + extra, exit_on_error=False)
        assert np.array_equal(a[3], plain[3]) and a[7] == plain[7] == 20
    assert not os.path.exists(g + ".ecg")


def test_without_c_the_ecg_flags_are_parsed_and_checked_before_anything_runs(tmp_path, monkeypatch):
    import cge.jl_amd as cg
    from cge.jl_amd import clustering
    from cge.jl_amd.args import USAGE, ParseError

    g, c, e = _files(tmp_path)
    for extra, word in ((["--ecg", "--louvain-level", "2"], "exclude"), (["--ecg", "8", "--louvain-level", "-1"], "exclude"),
                        (["--ecg", "65"], "members"), (["--ecg", "0"], "members"), (["--ecg", "--ecg-wmin", "1.0"], "--ecg-wmin"),
                        (["--ecg", "--ecg-wmin", "-0.5"], "--ecg-wmin")):
        with pytest.raises(ParseError, match=word):
            cg.parseargs(["-g", g, "-e", e] + extra, exit_on_error=False)
    assert not os.path.exists(g + ".ecg")
    assert "--ecg [members]" in USAGE and "--ecg-wmin" in USAGE
    seen = []

    def fake(*args, **kw):  # what parseargs hands to ecg_clust; the communities file is the fixture's
        seen.append((args, kw))
        shutil.copy(c, g + ".ecg")

    monkeypatch.setattr(clustering, "ecg_clust", fake)
    for extra, want in ((["--ecg"], dict(members=16, w_min=0.05, seed=0)), (["--ecg", "-l", "20"], dict(members=16, w_min=0.05, seed=0)),
                        (["--ecg", "8", "--seed", "3"], dict(members=8, w_min=0.05, seed=3)),
                        (["--ecg", "nonsense", "--ecg-wmin", "0.25", "--seed", "-4"], dict(members=16, w_min=0.25, seed=-4))):
        cg.parseargs(["-g", g, "-e", e] + extra, exit_on_error=False)
        assert seen[-1] == ((0.0, g), want), (extra, seen[-1])
    assert len(seen) == 4
