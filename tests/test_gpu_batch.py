"""cge_score_batch / Context.score_batch on the GPU (`pytest -m gpu`): a batch must give, member by member, what separate
cge_score calls give on the same context -- the same bits of the vector, the same div / auc traces, the same Chung-Lu
iteration counts -- whether the members' sweeps shared their launches (undirected landmark mode, the fused fit) or were scored
one after another (directed), and whatever the batch is made of (several launch groups, members of different landmark counts,
members that stop at different alphas, abandoned persistent fits).  Transitively against the oracle: a member at config 2's
shape matches oracle_cfg2.npz as the config test does."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


_CASES = {}


def _case(n=20000, C=20, d=16, seed=21):
    """An ABCD-like graph with dyadic weights (order-free scatter sums) and K-ready embeddings of it."""
    key = (n, C, d, seed)
    if key not in _CASES:
        from cge.jl_amd import synth

        g = synth.abcd_like(n, 10 * n, C, d, seed=seed)
        rng = np.random.default_rng(seed)
        ew = rng.integers(1, 17, size=len(g["eweights"])) / 4.0
        vw = np.zeros(n)
        np.add.at(vw, g["edges"][:, 0] - 1, ew)
        np.add.at(vw, g["edges"][:, 1] - 1, ew)
        _CASES.clear()
        _CASES[key] = (g, ew, vw)
    return _CASES[key]


def _embeddings(g, K, seed=0):
    """K embeddings of one graph that score differently: the graph's own, noisier copies of it, and one without structure."""
    rng = np.random.default_rng(seed)
    X = np.asarray(g["embedding"])
    out = [X]
    for k in range(1, K):
        if k == K - 1 and K >= 3:
            out.append(np.asfortranarray(rng.standard_normal(X.shape)))
        else:
            out.append(np.asfortranarray(X + (0.4 * k) * rng.standard_normal(X.shape)))
    return out


def _separate(ctx, embs, clusters, land, **kw):
    res, trs = [], []
    for e in embs:
        ctx.set_embedding(e)
        res.append(ctx.score(clusters, land, **kw))
        trs.append(ctx.last_trace)
    return res, trs


def _assert_same(got, got_tr, exp, exp_tr):
    assert len(got) == len(exp)
    for k in range(len(exp)):
        assert np.array_equal(got[k], exp[k]), (k, got[k], exp[k])
        assert got_tr[k]["n_alpha"] == exp_tr[k]["n_alpha"] and got_tr[k]["iters"] == exp_tr[k]["iters"], k
        assert np.array_equal(got_tr[k]["div"], exp_tr[k]["div"], equal_nan=True), k
        assert np.array_equal(got_tr[k]["auc"], exp_tr[k]["auc"], equal_nan=True), k


def _setup(ctx, g, ew, vw):
    ctx.set_graph(g["edges"], ew, g["n"])
    ctx.set_vertex_data(g["comm"], vw)


@pytest.mark.parametrize("seed,split", [(5, False), (-1, False), (7, True)])
def test_batch_of_four_at_400_landmarks_equals_separate_scores(ctx, seed, split):
    g, ew, vw = _case()
    _setup(ctx, g, ew, vw)
    embs = _embeddings(g, 4, seed=1)
    kw = dict(forced=4, method="rss", split=split, seed=seed, auc_samples=6000)
    got = ctx.score_batch(embs, g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    launches, alphas = ctx.get_stat("fit_batched_launches"), ctx.get_stat("fit_batched_alphas")
    exp, exp_tr = _separate(ctx, embs, g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)
    n_alpha = [t["n_alpha"] for t in exp_tr]
    assert alphas == sum(n_alpha)  # every member-alpha was fitted by a shared launch ...
    assert launches < sum(n_alpha)  # ... and the launches really were shared
    assert len(set(n_alpha)) > 1, n_alpha  # members stop at different alphas: the drop-out ran


def test_batch_in_two_launch_groups_with_members_of_different_landmark_counts(ctx):
    """K = 6 at -l 1000: 64 workgroups per member, four per launch group on 256 CUs -> two groups.  Member 2 has only 300
    distinct rows, so the unique-row clamp lowers its landmark count below the others' and it rides in a launch beside
    members of N = 1000."""
    g, ew, vw = _case()
    _setup(ctx, g, ew, vw)
    embs = _embeddings(g, 6, seed=2)
    rng = np.random.default_rng(3)
    X = np.asarray(g["embedding"])
    embs[2] = np.asfortranarray(X[rng.integers(0, 300, size=g["n"])])
    kw = dict(forced=4, method="rss", seed=11, auc_samples=6000)
    got = ctx.score_batch(embs, g["clusters"], 1000, **kw)
    got_tr = ctx.last_traces
    launches = ctx.get_stat("fit_batched_launches")
    assert ctx.landmarks_info()[0] == 1000  # the last member's landmark state is the resident one
    Ns, exp, exp_tr = [], [], []
    for e in embs:
        ctx.set_embedding(e)
        exp.append(ctx.score(g["clusters"], 1000, **kw))
        exp_tr.append(ctx.last_trace)
        Ns.append(ctx.landmarks_info()[0])
    assert 256 <= Ns[2] <= 300 and all(N == 1000 for k, N in enumerate(Ns) if k != 2), Ns
    _assert_same(got, got_tr, exp, exp_tr)
    assert launches < sum(t["n_alpha"] for t in exp_tr)


def test_batch_with_abandoned_persistent_fits_equals_separate_scores(ctx):
    g, ew, vw = _case()
    _setup(ctx, g, ew, vw)
    embs = _embeddings(g, 3, seed=4)
    kw = dict(forced=4, method="rss", seed=3, auc_samples=6000)
    ctx.set_option("fit_persistent_test_timeout", 1)
    try:
        got = ctx.score_batch(embs, g["clusters"], 400, **kw)
        got_tr = ctx.last_traces
        assert ctx.get_stat("fit_batched_alphas") == 0  # every member fell back to cge_score's own path
        exp, exp_tr = _separate(ctx, embs, g["clusters"], 400, **kw)
    finally:
        ctx.set_option("fit_persistent_test_timeout", 0)
    _assert_same(got, got_tr, exp, exp_tr)


def test_directed_batch_equals_separate_scores(ctx):
    from cge.jl_amd import synth

    g = synth.abcd_like(3000, 24000, 6, 8, seed=3, directed=True)
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    embs = _embeddings(g, 3, seed=5)
    kw = dict(forced=4, method="rss", directed=True, seed=2, auc_samples=4000)
    got = ctx.score_batch(embs, g["clusters"], 100, **kw)
    got_tr = ctx.last_traces
    assert ctx.get_stat("fit_batched_launches") == 0  # (the directed sweep is not batched)
    exp, exp_tr = _separate(ctx, embs, g["clusters"], 100, **kw)
    _assert_same(got, got_tr, exp, exp_tr)


def test_batch_with_a_homogeneous_member_raises_and_leaves_the_context_usable(ctx):
    """The construction of test_gpu_parity.py::test_score_that_fails_between_the_halves_of_its_sample_draw as the FIRST member:
    it raises after its sample draw was enqueued.  Right after, a draw, a batch of the good members and a score all work."""
    from cge.jl_amd import api

    g, ew, _ = _case()
    n, d = g["n"], g["embedding"].shape[1]
    ctx.set_graph(g["edges"], ew, n)
    ctx.set_vertex_data(g["comm"], np.full(n, 2.0))
    bad = np.tile(np.arange(1.0, d + 1.0), (n, 1))
    good = _embeddings(g, 2, seed=6)
    kw = dict(forced=4, method="rss", seed=1, auc_samples=5000)
    with pytest.raises(api.CGEError, match="homogenous"):
        ctx.score_batch([bad] + good, g["clusters"], 400, **kw)
    smp = ctx.draw_samples(1, 5000)
    assert len(smp[0]) == 5000
    got = ctx.score_batch(good, g["clusters"], 400, **kw)
    got_tr = ctx.last_traces
    assert ctx.get_stat("fit_batched_alphas") > 0
    exp, exp_tr = _separate(ctx, good, g["clusters"], 400, **kw)
    _assert_same(got, got_tr, exp, exp_tr)


def test_batch_member_at_config2_shape_against_oracle_fixture(ctx):
    """bench.py's cfg2 (10^5 vertices, d = 64, -l 400 -m rss2, seed 42): the last member of a batch of two is the fixture's
    embedding; its landmarks (resident after the call) and its sweep match oracle_cfg2.npz as the config test checks them."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_configs import _check_landmarks, _check_sweep, _fixture, crc
    from cge.jl_amd import synth

    fx = _fixture("cfg2")
    g = synth.abcd_like(100_000, 1_050_000, 50, 64, seed=42)
    assert crc(g["edges"]) == int(fx["edges_crc"]) and crc(g["embedding"]) == int(fx["emb_crc"])
    ctx.set_graph(g["edges"], g["eweights"], g["n"])
    ctx.set_vertex_data(g["comm"], g["vweights"])
    ctx.set_option("diameter", 0)
    other = np.asfortranarray(np.asarray(g["embedding"]) + 0.3 * np.random.default_rng(8).standard_normal(g["embedding"].shape))
    res = ctx.score_batch([other, g["embedding"]], g["clusters"], 400, 4, "rss2", seed=42, auc_samples=10000)
    tr = ctx.last_traces[1]
    assert ctx.get_stat("fit_batched_alphas") == sum(t["n_alpha"] for t in ctx.last_traces)
    _check_landmarks(ctx, fx)
    _check_sweep(res[1], tr, fx, same_samples=False)
    assert np.array_equal(res[1], ctx.score(g["clusters"], 400, 4, "rss2", seed=42, auc_samples=10000))


def test_compare_script_first_line_equals_cli(tmp_path):
    g = os.path.join(GOLDEN, "example10k")
    emb = np.loadtxt(os.path.join(g, "10k.embedding"))
    rng = np.random.default_rng(9)
    pert = emb.copy()
    pert[:, 1:] += 0.25 * rng.standard_normal(pert[:, 1:].shape)
    other = os.path.join(tmp_path, "10k_perturbed.embedding")
    np.savetxt(other, pert, fmt=["%d"] + ["%.17g"] * (pert.shape[1] - 1))
    flags = ["-g", f"{g}/10k.edgelist", "-c", f"{g}/10k.ecg", "-l", "400", "--seed", "42"]
    env = dict(os.environ)
    cli = subprocess.run([sys.executable, os.path.join(ROOT, "cge_cli.py"), *flags, "-e", f"{g}/10k.embedding"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert cli.returncode == 0, cli.stderr[-2000:]
    cmp_ = subprocess.run([sys.executable, os.path.join(ROOT, "cge_compare.py"), *flags, "-e", f"{g}/10k.embedding", "-e", other],
                          capture_output=True, text=True, timeout=300, env=env)
    assert cmp_.returncode == 0, cmp_.stderr[-2000:]
    lines = cmp_.stdout.strip().split("\n")
    assert len(lines) == 2
    assert lines[0] == f"{g}/10k.embedding\t{cli.stdout.strip()}"
    assert lines[1].startswith(other + "\t[") and lines[1] != lines[0]
