"""CPU tests of cge_link_sample's reference (tests/link_sample_ref.py), of the inputs the GPU tests rely on, and of the feature's
presence in the header, the built library and the command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import link_ref as lr
import link_sample_ref as sr
import local_score_ref as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uniform_is_the_scalar_stream_element_by_element():
    rng = np.random.default_rng(1)
    seeds = [0, 1, 42, -1, 2 ** 63 - 1] + rng.integers(0, 2 ** 62, 5).tolist()
    streams = [0, 1, 7, 1000, 2 ** 40]
    n = 0
    for seed in seeds:
        for stream in streams:
            a = np.concatenate([[0, 1, 127, 128, 2 ** 31 - 1], rng.integers(0, 10 ** 6, 4)]).astype(np.int64)
            b = np.concatenate([[1, 0, 128, 127, 2 ** 31 - 2], rng.integers(0, 10 ** 6, 4)]).astype(np.int64)
            got = sr.rand64(seed, stream, a, b)
            for q in range(len(a)):
                assert int(got[q]) == ls.ctr_rand(seed, stream, int(a[q]), int(b[q]), sr.WHICH)
                n += 1
            u = sr.uniform(seed, stream, a, b)
            assert [float(x) for x in u] == [(ls.ctr_rand(seed, stream, int(x), int(y), 5) >> 11) * 2.0 ** -53 for x, y in zip(a, b)]
    assert n >= 300


def test_uniform_lies_in_the_unit_interval_and_looks_uniform():
    n = 1000
    U = sr.uniform_matrix(3, 0, n)
    assert U.min() >= 0.0 and U.max() < 1.0
    N = n * n
    # the mean of N uniforms has sigma sqrt(1 / (12 N)); the share below 0.3 has sigma sqrt(0.21 / N)
    assert abs(U.mean() - 0.5) <= 5 * np.sqrt(1.0 / (12 * N))
    assert abs((U < 0.3).mean() - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / N)


def test_draws_are_distinct():
    n = 300
    U0, U1 = sr.uniform_matrix(3, 0, n), sr.uniform_matrix(3, 1, n)
    off = ~np.eye(n, dtype=bool)
    assert (U0 != U0.T)[off].all()  # (a, b) and (b, a)
    assert (U0 != U1).all()         # stream 0 and stream 1
    assert (U0 != sr.uniform_matrix(4, 0, n)).all()


def test_the_set_of_a_matrix():
    i, j = sr.all_pairs(3, True)
    assert list(zip(i, j)) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert list(zip(*sr.all_pairs(3, False))) == [(0, 1), (0, 2), (1, 2)]
    p = np.array([0.5, 0.0, 1.0, 2.0, 0.25, 0.25])
    u = np.array([0.5, 0.0, 0.999, 0.0, 0.2499, 0.25])
    ei, ej, ep = sr.sampled(i, j, p, u)
    assert list(zip(ei, ej)) == [(1, 0), (1, 2), (2, 0)] and ep.tolist() == [1.0, 2.0, 0.25]


@pytest.mark.parametrize("shape", [s for s in sr.SHAPES if s[0] >= 127], ids=sr.shape_id)
def test_the_inputs_have_what_the_gpu_tests_rely_on(shape):
    """Between 1 % and 60 % of the pairs are edges under the long-double reference; a diagonal tile holds edges and non-edges,
    and so does an off-diagonal tile wherever there is one (n > 128: with n <= 128 the whole matrix is one diagonal tile)."""
    n, d, directed = shape
    c = sr.shape_case(*shape)
    i, j = sr.all_pairs(n, directed)
    p = lr.prob(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], i, j)
    e = sr.uniform(0, 0, i, j) < p
    share = e.mean()
    assert 0.01 <= share <= 0.60, share
    assert (p > 1).any() and (p == 0).any()
    ti, tj = i // 128, j // 128
    diag = ti == tj
    assert e[diag].any() and (~e[diag]).any()
    if n > 128:
        assert e[~diag].any() and (~e[~diag]).any()
        if directed:
            assert e[ti > tj].any() and (~e[ti > tj]).any()  # the tiles below the diagonal, which only a directed draw walks
    mean_p = float(np.minimum(p, 1).mean())
    assert 0.02 <= mean_p <= 0.12, mean_p


def test_the_small_shapes_have_pairs_of_positive_probability():
    for shape in (s for s in sr.SHAPES if s[0] < 127):
        c = sr.shape_case(*shape)
        i, j = sr.all_pairs(shape[0], shape[2])
        assert len(i) == (0 if shape[0] == 1 else 2 if shape[2] else 1) and len(c["edges"]) >= 1
        assert (lr.prob(c["X"], c["hi"], c["alpha"], c["fo"], c["fi"], i, j) > 0).all()


def test_the_threshold_cases_have_a_clamped_base_where_asked():
    for directed in (False, True):
        c = sr.threshold_case(300, directed, True)
        i, j = sr.all_pairs(300, directed)
        b = lr.base(c["X"], i, j, c["hi"])
        assert (b == 0).mean() > 0.2 and (b > 0).mean() > 0.02
        c = sr.threshold_case(300, directed, False)
        assert (lr.base(c["X"], i, j, c["hi"]) > 0).mean() > 0.99


# ---- the feature is present (no GPU) ----------------------------------------------------------------------------------------------
def test_cge_link_sample_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cge_hip.h")).read()
    assert "int cge_link_sample(cge_ctx *ctx, int64_t seed, int64_t stream, int64_t cap" in hdr
    assert "cge_link_sample_test(" in open(os.path.join(ROOT, "include", "cge_hip_testing.h")).read()
    from cge.jl_amd import api

    L = api.load_library()
    assert hasattr(L, "cge_link_sample") and hasattr(L, "cge_link_sample_test")
    # a NULL context or a NULL n_edges is refused at the door, without a device
    assert L.cge_link_sample(None, C.c_int64(0), C.c_int64(0), C.c_int64(0), None, None, None, None) == -7


def test_link_args_take_sample(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import cge_links as cl
    finally:
        sys.path.pop(0)
    base = ["-g", "g", "-c", "c", "-e", "e"]
    out = str(tmp_path / "sample.txt")
    plain = {"which": "local", "topk": 10, "queries": None, "pairs": None, "exclude": True}
    assert cl.link_args(base) == plain
    assert cl.link_args(base + ["--sample", out]) == dict(plain, sample=out, sample_seed=0)
    assert cl.link_args(base + ["--sample", out, "--sample-seed", "9"]) == dict(plain, sample=out, sample_seed=9)
    f = tmp_path / "f.txt"
    f.write_text("0 1\n")
    for bad in (["--sample"], ["--sample", out, "--rank", str(f)], ["--sample", out, "--pairs", str(f)],
                ["--sample", out, "--queries", str(f)], ["--sample", out, "--sample-seed", "x"], ["--sample-seed", "3"]):
        with pytest.raises(cl.LinkArgError):
            cl.link_args(base + bad)
