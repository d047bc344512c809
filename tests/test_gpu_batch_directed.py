"""cge_score_batch on a DIRECTED graph (`pytest -m gpu`): from 256 landmarks on, the members' Chung-Lu fits of an alpha share one
launch (fit_flow_dir_multi_kernel), and a batch still gives, member by member, what separate cge_score calls give on the same
context -- the same bits of the vector, the same div / auc traces, the same iteration counts.  Below 256 landmarks nothing is
shared (tests/test_gpu_batch.py::test_directed_batch_equals_separate_scores keeps that)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_batch import _assert_same, _embeddings, _separate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


_G = {}


def _graph(ctx):
    """A directed ABCD-like graph of 10^4 vertices, resident on the context."""
    if not _G:
        from cge.jl_amd import synth

        _G["g"] = synth.abcd_like(10000, 100000, 20, 16, seed=31, directed=True)
    g = _G["g"]
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    return g


def _batched(ctx):
    return ctx.get_stat("fit_batched_launches"), ctx.get_stat("fit_batched_alphas")


@pytest.mark.parametrize("seed,split", [(5, False), (-1, False), (7, True)])
def test_directed_batch_of_four_at_400_landmarks_shares_its_fits(ctx, seed, split):
    g = _graph(ctx)
    embs = _embeddings(g, 4, seed=1)
    kw = dict(forced=4, method="rss", directed=True, split=split, seed=seed, auc_samples=6000)
    got = ctx.score_batch(embs, g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    launches, alphas = _batched(ctx)
    assert ctx.landmarks_info()[0] == 400
    exp, exp_tr = _separate(ctx, embs, g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)
    n_alpha = [t["n_alpha"] for t in exp_tr]
    print("  n_alpha", n_alpha, "launches", launches, "member-alphas", alphas)
    assert alphas == sum(n_alpha)  # every member-alpha was fitted by a shared launch ...
    assert 0 < launches < sum(n_alpha)  # ... and the launches really were shared
    assert len(set(n_alpha)) > 1, n_alpha  # members stop at different alphas: the drop-out ran


def test_directed_batch_in_two_launch_groups_with_members_of_different_landmark_counts(ctx):
    """K = 6 at -l 1000: 64 workgroups per member on 256 CUs.  Member 2 has only 300 distinct rows, so the unique-row clamp
    lowers its landmark count and it rides (on 20 workgroups or fewer) beside members of N = 1000: groups of four and two."""
    g = _graph(ctx)
    embs = _embeddings(g, 6, seed=2)
    X = np.asarray(g["embedding"])
    embs[2] = np.asfortranarray(X[np.random.default_rng(3).integers(0, 300, size=g["n"])])
    kw = dict(forced=4, method="rss", directed=True, seed=11, auc_samples=6000)
    got = ctx.score_batch(embs, g["clusters"], 1000, **kw)
    got_tr = ctx.last_traces
    launches, alphas = _batched(ctx)
    assert ctx.landmarks_info()[0] == 1000  # the last member's landmark state is the resident one
    Ns, exp, exp_tr = [], [], []
    for e in embs:
        ctx.set_embedding(e)
        exp.append(ctx.score(g["clusters"], 1000, **kw))
        exp_tr.append(ctx.last_trace)
        Ns.append(ctx.landmarks_info()[0])
    assert 256 <= Ns[2] <= 300 and all(N == 1000 for k, N in enumerate(Ns) if k != 2), Ns
    _assert_same(got, got_tr, exp, exp_tr)
    n_alpha = [t["n_alpha"] for t in exp_tr]
    assert alphas == sum(n_alpha) and 0 < launches < sum(n_alpha)
    import torch

    if torch.cuda.get_device_properties(0).multi_processor_count == 256:  # two groups: each runs as long as its longest member
        assert launches == max(n_alpha[:4]) + max(n_alpha[4:]), (launches, n_alpha)


def test_directed_members_have_no_sample_ceiling(ctx):
    g = _graph(ctx)
    embs = _embeddings(g, 2, seed=3)
    kw = dict(forced=4, method="rss", directed=True, seed=9, auc_samples=70000)
    got = ctx.score_batch(embs, g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    launches, alphas = _batched(ctx)
    exp, exp_tr = _separate(ctx, embs, g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)
    assert alphas == sum(t["n_alpha"] for t in exp_tr) and launches > 0


def test_directed_batch_with_abandoned_persistent_fits_equals_separate_scores(ctx):
    g = _graph(ctx)
    embs = _embeddings(g, 3, seed=4)
    kw = dict(forced=4, method="rss", directed=True, seed=3, auc_samples=6000)
    ctx.set_option("fit_persistent_test_timeout", 1)
    try:
        got = ctx.score_batch(embs, g["clusters"], 400, **kw)
        got_tr = ctx.last_traces
        assert ctx.get_stat("fit_batched_alphas") == 0  # every member fell back to cge_score's own path
        exp, exp_tr = _separate(ctx, embs, g["clusters"], 400, **kw)
    finally:
        ctx.set_option("fit_persistent_test_timeout", 0)
    _assert_same(got, got_tr, exp, exp_tr)


def test_directed_batch_without_the_persistent_fit_shares_nothing(ctx):
    g = _graph(ctx)
    embs = _embeddings(g, 2, seed=5)
    kw = dict(forced=4, method="rss", directed=True, seed=4, auc_samples=6000)
    ctx.set_option("fit_persistent", 1)
    try:
        got = ctx.score_batch(embs, g["clusters"], 400, **kw)
        got_tr = ctx.last_traces
        assert _batched(ctx) == (0, 0)
        exp, exp_tr = _separate(ctx, embs, g["clusters"], 400, **kw)
    finally:
        ctx.set_option("fit_persistent", 0)
    _assert_same(got, got_tr, exp, exp_tr)


def test_directed_score_views_of_different_members_shares_its_fits(ctx):
    """An fp32 device tensor of d = 8 next to an fp64 host matrix of d = 16."""
    import torch

    g = _graph(ctx)
    X = np.asarray(g["embedding"])
    rng = np.random.default_rng(6)
    m0 = torch.from_numpy(np.ascontiguousarray(X[:, :8] + 0.3 * rng.standard_normal((g["n"], 8)), dtype=np.float32)).cuda()
    m1 = np.asfortranarray(X)
    wid = [m0.cpu().to(torch.float64).numpy(), m1]
    kw = dict(forced=4, method="rss", directed=True, seed=2, auc_samples=6000)
    got = ctx.score_views([m0, m1], g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    launches, alphas = _batched(ctx)
    exp, exp_tr = _separate(ctx, wid, g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)
    n_alpha = [t["n_alpha"] for t in exp_tr]
    assert alphas == sum(n_alpha) and 0 < launches < sum(n_alpha)


def test_compare_script_directed_prints_what_the_cli_prints(tmp_path):
    g = os.path.join(GOLDEN, "example10k")
    emb = np.loadtxt(os.path.join(g, "10k.embedding"))
    pert = emb.copy()
    pert[:, 1:] += 0.25 * np.random.default_rng(9).standard_normal(pert[:, 1:].shape)
    other = os.path.join(tmp_path, "10k_perturbed.embedding")
    np.savetxt(other, pert, fmt=["%d"] + ["%.17g"] * (pert.shape[1] - 1))
    flags = ["-g", f"{g}/10k.edgelist", "-c", f"{g}/10k.ecg", "-l", "400", "--seed", "42", "-d"]
    files = [f"{g}/10k.embedding", other]
    env = dict(os.environ)
    cmp_ = subprocess.run([sys.executable, os.path.join(ROOT, "cge_compare.py"), *flags, "-e", files[0], "-e", files[1]],
                          capture_output=True, text=True, timeout=300, env=env)
    assert cmp_.returncode == 0, cmp_.stderr[-2000:]
    lines = cmp_.stdout.strip().split("\n")
    assert len(lines) == 2 and lines[0] != lines[1]
    for f, line in zip(files, lines):
        cli = subprocess.run([sys.executable, os.path.join(ROOT, "cge_cli.py"), *flags, "-e", f], capture_output=True, text=True,
                             timeout=300, env=env)
        assert cli.returncode == 0, cli.stderr[-2000:]
        assert line == f"{f}\t{cli.stdout.strip()}"
