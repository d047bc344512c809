"""The sharded paths (options shard_ingest, shard_rows, shard_samples, shard_runsplit) at the shapes where sharding rules go
wrong: worlds of 2, 3 and 5 ranks on the one GPU of the test box, graphs of a few vertices, odd sample counts, communities of one
row, more ranks than chunks, rows or communities (run with -m gpu on an MI355X).  tests/test_gpu_two_ranks.py holds the same
options on one 30 000-vertex graph at W = 2 (one case of 4) through whole-run outputs; here the stages of the local score run
under shards one by one through the testing hook's opt-in (cge_local_score_test, `sharded` = 1), next to small whole runs.

The ranks of a world are started ONCE (tests/rank_workers.py) and run the cases of CASES in lock-step; every test below judges one
case's recorded results, so a failure names the shape.  References: tests/local_score_ref.py (the counter stream, prepare, dist())
and a one-rank context in the parent; tests/test_gpu_local_score.py holds the one-rank kernels to the same reference.  Edge weights
are unit or dyadic, so every sum is exact in any grouping.

Graphs (built here with numpy, the same in every process):
  pair      n = 9, m = 12, C = 2, d = 2            C == W at W = 2; fewer communities than ranks at W = 3, 5
  tiny      n = 7, m = 9, C = 3, d = 1             C == W at W = 3; fewer communities than ranks at W = 5
  tiny5     n = 11, m = 14, C = 5, d = 1           stands in for `tiny` at W = 5, where shard_rows refuses C = 3 (see below)
  odd       n = 301, m = 1501, C = 5, d = 17       communities of 200 / 60 / 30 / 10 / 1 rows: at W = 5 one rank owns ONE row, at
            W = 2 one rank owns 200 of 301; -0.0 entries (the last row's among them); `odd_dir` its directed twin, `odd_w` weighted
  wide      n = 130, m = 700, C = 6, d = 512
  few40     n = 40, m = 2;  few3: n = 3, m = 2     fewer edges / rows than ranks
  sparse    n = 5801, m = 1501 (weighted: sparse_w); bigfew: n = 5801, m = 2; dense: n = 5801, every pair with (i + j) % 8 == 0
            (2.1 million edges, 12.5 % of the pairs: the rejection loop of the sampler runs four or five rounds at S = 4001)

Rules of the library that decide which of the issue's shapes exist (read in graph_host.cpp, wgcl_host.cpp, embedding_host.cpp), and
what stands in their place:
  * set_graph shards the edge list under shard_ingest only when n (n - 1) > 2^25 -- below, the sampler enumerates the non-edges on
    the host and needs the whole list -- AND m >= W.  So the exchange variants of Draw and Prepare cannot run on tiny / odd / wide /
    few*: they run on `sparse` and `dense`, n = 5801 being the first odd n past the rule; on the small graphs the same calls are
    made and take the one-rank kernels (asserted through edges_resident == edges_total).
  * For the same reason NO rank ever holds an empty edge slice: m < W keeps the list whole on every rank (few40, few3, bigfew at
    W = 3, 5: edges_resident == 2 everywhere, the results those of one rank).  The empty share that does exist is the CHUNK share
    of a replicated list: one chunk of the blocked edge list over W ranks leaves W - 1 ranks the "an empty shard still owes zeros"
    branch of k_edge_scatter_blocked -- asserted by stat edge_chunks < W in every whole run here, which scores twice on one context
    so that the second run meets the first run's sums in the buffer.
  * The tallies are split (shard_samples = 2) only when S >= W: auc_samples = 3 is split at W = 2, 3 (one or two samples a rank)
    and runs unsplit at W = 5; no rank ever tallies an empty range.
  * shard_rows refuses fewer non-empty communities than ranks: `tiny` (C = 3) at W = 5 and `pair` (C = 2) at W = 3, 5 are the
    refusal cases, `tiny5` carries d = 1 through the row exchange at W = 5.
  * An embedding slice under shard_ingest IS empty when n < W (few3 at W = 5: ranks 3 and 4 upload nothing and still all-gather).

The refusal that diverged: rows_assign_ownership raised "fewer communities than ranks" only on the rank that would own no row; the
others went on into the all-reduce of the column sums and waited there.  Now every rank refuses when any rank's load is zero
(embedding_host.cpp), with the same code and message; test_fewer_communities_than_ranks_is_refused_on_every_rank holds that and
that the context is usable afterwards.

The bug these shapes found: forced_over_ranks (W > 1, shard_runsplit >= 1, forced >= 2, rows not sharded) rewrote the start of the
member arena from the gathered words, but no rank entered the communities of at most `forced` rows (they own no local heap): the
one-row community of `odd` came back as vertex 0 and the landmark index refused ("all(>=(0), group_ids)") on every rank.  Rank 0
enters them now (landmarks_host.cpp); the `ingest` and `none` whole runs on `odd` hold it.

Measured on an MI355X (`-s` prints them, test_times_are_reported): the ranks' start-up 2.7 s (W = 2), 2.8 s (W = 3), 2.8 s (W = 5);
their cases 2.0 s, 3.0 s and 3.7 s in all (the slowest case, a directed whole run on 5 ranks, 0.5 s); a world from the first
start() to the last join 5.7 s, 7.3 s and 7.9 s; the whole file 22.5 s for 179 tests -- tests/test_gpu_two_ranks.py took 68.7 s
for its 23 in the same run.

Scratch mutants of the library (tried on a copy, not committed; each run stopped at its first failure) and the test that noticed:
  prep_store_sharded_kernel without the `- 1`         test_two_edges_on_many_vertices[2] (pi of sample 1); by reading, every case of
                                                      test_prepared_pairs_over_a_sharded_edge_list too
  check_neg_flag_kernel reading `flag[idx]`           test_draws_over_a_sharded_edge_list from S = 3 on (sample 2 keeps a pair that
                                                      is an edge: its verdict was read at the wrong index in round 1)
  `S / 2` words exchanged in draw_round               test_draws_over_a_sharded_edge_list at S = 1 already: the last sample's verdict
                                                      stays rank-local, the ranks run different numbers of rounds, the exchange of
                                                      the rank left alone times out (CGE_E_COLLECTIVE in its record), the world
                                                      stops and names the case -- 113 s a world, not a stuck run
  pair_dist_rows_kernel reading row 2k for both ends  the chained distances of test_prepared_pairs_over_a_sharded_edge_list (`both`),
                                                      by reading, test_pair_distances_through_the_row_exchange too (every distance 0)
  the empty-shard memset of k_edge_scatter_blocked    test_small_whole_runs_reproduce_one_rank, from its first case on (element 0 of
  removed                                             the vector is -1, the divergences inf)
"""
import functools

import numpy as np
import pytest

import local_score_ref as ls
import rank_workers as rw

pytestmark = pytest.mark.gpu

WORLDS = (2, 3, 5)
SEED = 11
HI = 7.25
E_ARG = -7
DRAW_S = (1, 2, 3, 255, 257, 4001)
OPTS = {"none": (), "ingest": (("shard_ingest", 1),), "rows": (("shard_rows", 1),),
        "both": (("shard_ingest", 1), ("shard_rows", 1))}
STATS = ("edges_resident", "edges_total", "edge_chunks", "rows_resident", "rows_total")


# ---- the graphs ----------------------------------------------------------------------------------------------------------------
def _finish(n, rows, comm0, emb, directed, weighted):
    m = len(rows)
    ew = 1.0 + (np.arange(m) % 4) * 0.25 if weighted else np.ones(m)
    vw = np.zeros(n)
    np.add.at(vw, rows[:, 0], ew)
    np.add.at(vw, rows[:, 1], ew)
    C = int(comm0.max()) + 1
    return {"edges": np.asfortranarray(rows + 1), "rows0": rows, "eweights": ew, "vweights": vw, "comm0": comm0,
            "comm": np.asfortranarray((comm0 + 1).reshape(-1, 1)), "clusters": [np.flatnonzero(comm0 == q) + 1 for q in range(C)],
            "embedding": np.asfortranarray(emb), "n": n, "m": m, "d": emb.shape[1], "C": C, "directed": directed,
            "weighted": weighted}


def _build(n, sizes, d, m, seed, directed=False, weighted=False, neg_zero=False):
    rng = np.random.default_rng(seed)
    C = len(sizes)
    assert sum(sizes) == n
    comm0 = np.repeat(np.arange(C), sizes)[rng.permutation(n)]
    members = [np.flatnonzero(comm0 == q) for q in range(C)]
    pairs = set()
    if m >= n:  # a ring first: no isolated vertex (a zero vertex weight would put a NaN into a score)
        for i in range(n):
            pairs.add((min(i, (i + 1) % n), max(i, (i + 1) % n)))
    while len(pairs) < m:
        a = int(rng.integers(n))
        b = int(rng.choice(members[comm0[a]])) if rng.random() < 0.7 else int(rng.integers(n))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    rows = np.array(sorted(pairs), np.int64)
    rows[1::3] = rows[1::3][:, ::-1]  # every third row stored as (max, min): an undirected list may hold either
    if directed:  # the twin: the same pairs, every second one or so turned round
        flip = np.random.default_rng(seed + 1000).random(m) < 0.5
        rows[flip] = rows[flip][:, ::-1]
    emb = rng.standard_normal((C, d))[comm0] * 2.0 + rng.standard_normal((n, d)) * 0.5
    if neg_zero:
        emb[3::41, min(2, d - 1)] = -0.0
        emb[n - 1, d - 1] = -0.0
        emb[n - 1, 0] = -0.0
    return _finish(n, rows, comm0, emb, directed, weighted)


def _dense_pred(i, j):  # undirected, 12.5 % of the pairs
    return (i + j) % 8 == 0


def _build_dense(n=5801):
    js = [np.arange(i + 1 + (-(2 * i + 1)) % 8, n, 8, dtype=np.int64) for i in range(n)]  # the j > i with (i + j) % 8 == 0
    rows = np.stack((np.repeat(np.arange(n, dtype=np.int64), [len(j) for j in js]), np.concatenate(js)), axis=1)
    flip = (rows[:, 0] // 3 + rows[:, 1]) % 2 == 1  # every second row or so stored as (max, min)
    rows[flip] = rows[flip][:, ::-1]
    comm0 = np.arange(n) % 5
    emb = np.stack((np.arange(n) % 7, np.arange(n) % 3), axis=1) * 0.5
    return _finish(n, rows, comm0, emb, False, False)


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "pair":
        return _build(9, (5, 4), 2, 12, 7)
    if name == "tiny":
        return _build(7, (3, 2, 2), 1, 9, 1)
    if name == "tiny5":
        return _build(11, (3, 2, 2, 2, 2), 1, 14, 8)
    if name in ("odd", "odd_dir", "odd_w"):
        return _build(301, (200, 60, 30, 10, 1), 17, 1501, 2, directed=name == "odd_dir", weighted=name == "odd_w", neg_zero=True)
    if name == "wide":
        return _build(130, (40, 30, 25, 20, 10, 5), 512, 700, 3)
    if name == "few40":
        return _build(40, (20, 10, 5, 3, 2), 3, 2, 4)
    if name == "few3":
        return _build(3, (1, 1, 1), 2, 2, 5)
    if name in ("sparse", "sparse_w"):
        return _build(5801, (3000, 1500, 800, 400, 101), 3, 1501, 6, weighted=name == "sparse_w")
    if name == "bigfew":
        return _build(5801, (3000, 1500, 800, 400, 101), 3, 2, 9)
    if name == "dense":
        return _build_dense()
    raise KeyError(name)


def _thin(world):  # the d = 1 graph a world accepts under shard_rows
    return "tiny" if world <= 3 else "tiny5"


def _edges_are_sharded(g, world):  # the rule of set_graph under shard_ingest
    return g["n"] * (g["n"] - 1) > 2 ** 25 and g["m"] >= world


def _owner(g, world):
    from cge.jl_amd.dist import community_owner

    return community_owner(g["comm"][:, 0], world)[g["comm0"]]  # the owner of every vertex


def _is_edge(g):
    keys = set((int(a) << 32) | int(b) for a, b in (g["rows0"] if g["directed"] else np.sort(g["rows0"], axis=1)))
    return lambda i, j: ((int(i) << 32) | int(j)) in keys


@functools.lru_cache(maxsize=None)
def _dense_stream(S):
    """The stream of the dense draw of S samples: the first whose LAST sample is rejected in round 0 (its first candidate is an
    edge), so that the verdict of sample S - 1 -- the odd one of the flag words when S is odd -- has to cross the ranks."""
    n = _graph("dense")["n"]
    return next(st for st in range(4096) if _dense_pred(*ls.candidate(SEED, st, S - 1, 0, n, False)))


def _load(ctx, g):
    ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])


def _draw_keys(o):
    return {k: o[k] for k in ("pos", "neg_i", "neg_j", "attempt", "rounds")}


# ---- the cases (run on every rank; they return, the parent judges) -----------------------------------------------------------
CASES, CASE_WORLDS = {}, {}


def _case(name, worlds=WORLDS):
    def deco(fn):
        CASES[name] = fn
        CASE_WORLDS[name] = tuple(worlds)
        return fn
    return deco


def _stats(ctx):
    return {k: int(ctx.get_stat(k)) for k in STATS}


RES_ROWS = [("pair", (2,)), ("tiny", (2, 3)), ("tiny5", (5,)), ("odd", WORLDS), ("wide", WORLDS)]
RES_INGEST = ["odd", "few40", "few3", "sparse_w", "bigfew"]


def _make_residents():
    for gname, worlds in RES_ROWS:
        for opt in ("rows", "both"):
            @_case(f"res_rows-{gname}-{opt}", worlds)
            def case(env, gname=gname, opt=opt):
                g = _graph(gname)
                ctx, _ = env.context(options=OPTS[opt])
                _load(ctx, g)
                rows, ids = ctx.resident_embedding()
                return dict(rows=rows, ids=ids, stats=_stats(ctx))
    for gname in RES_INGEST:
        @_case(f"res_ingest-{gname}")
        def case(env, gname=gname):
            g = _graph(gname)
            ctx, _ = env.context(options=OPTS["ingest"])
            _load(ctx, g)
            rows, ids = ctx.resident_embedding()
            rg = ctx.resident_graph()
            return dict(rows=rows, ids=ids, stats=_stats(ctx), src=rg["src"], dst=rg["dst"], w=rg["w"], unit=rg["unit"], m=rg["m"])


def _make_draws():
    for opt in ("ingest", "both"):
        @_case(f"draw_dense-{opt}")
        def case(env, opt=opt):
            g = _graph("dense")
            ctx, _ = env.context(options=OPTS[opt])
            _load(ctx, g)
            out = {(S, route): _draw_keys(ctx.local_score_test(S, draw=(SEED, _dense_stream(S), route), sharded=True))
                   for S in DRAW_S for route in (1, 2)}
            out["stats"] = _stats(ctx)
            return out
    for gname in ("odd", "odd_dir"):
        for opt in ("rows", "ingest", "both"):
            @_case(f"draw_prepare-{gname}-{opt}")
            def case(env, gname=gname, opt=opt):
                g = _graph(gname)
                ctx, _ = env.context(options=OPTS[opt])
                _load(ctx, g)
                out = {(S, route): ctx.local_score_test(S, directed=g["directed"], draw=(SEED, 0, route), prepare=True, sharded=True)
                       for S in (1, 257) for route in (1, 2)}
                out["stats"] = _stats(ctx)
                return out


def _prepare_samples(g, world):
    """Supplied draws over the WHOLE list: `own0` rows of rank 0's slice alone (so no sampled row touches any other rank), `last`
    rows of the last rank's slice alone, `mixed` rows of every slice, each with a second draw for pos2."""
    from cge.jl_amd.dist import edge_shard

    rng = np.random.default_rng(31)
    m, n, out = g["m"], g["n"], {}
    for key, (lo, hi), S in (("own0", edge_shard(m, 0, world), 257), ("last", edge_shard(m, world - 1, world), 3), ("mixed", (0, m), 1000)):
        pos, pos2 = rng.integers(lo, hi, S), rng.integers(lo, hi, S)
        ni, nj = rng.integers(0, n, S), rng.integers(0, n, S)
        if key == "mixed":
            pos[:world] = [edge_shard(m, r, world)[0] for r in range(world)]  # the first row of every slice,
            pos[world:2 * world] = [edge_shard(m, r, world)[1] - 1 for r in range(world)]  # and the last
            pos2[:world] = pos[:world][::-1]
        out[key] = (pos, pos2, ni, nj)
    return out


def _make_prepares():
    for gname in ("sparse", "sparse_w"):
        for opt in ("ingest", "both"):
            @_case(f"prepare-{gname}-{opt}")
            def case(env, gname=gname, opt=opt):
                g = _graph(gname)
                ctx, _ = env.context(options=OPTS[opt])
                _load(ctx, g)
                out = {}
                for key, (pos, pos2, ni, nj) in _prepare_samples(g, env.world).items():
                    for directed in (False, True):
                        for p2 in (None, pos2):
                            out[(key, directed, p2 is not None)] = ctx.local_score_test(
                                len(pos), directed=directed, draws=(pos, ni, nj), pos2=p2, prepare=True, sharded=True)
                # the stages chained: the pairs just drawn are prepared, and the prepared pairs are measured (a call of its own, so
                # that the hook's range checks stand between a wrong pair and the rows; both shardings: every exchange runs)
                ch = ctx.local_score_test(257, draw=(SEED, 3, 1), prepare=True, sharded=True)
                ch.update(ctx.local_score_test(257, pairs=tuple(ch[k] for k in ("pi", "pj", "ni", "nj", "wts")), hi=HI, distances=True,
                                               sharded=True))
                out["chain"] = ch
                out["stats"] = _stats(ctx)
                return out

    @_case("draw_prepare-bigfew-ingest")
    def case(env):
        g = _graph("bigfew")
        ctx, _ = env.context(options=OPTS["ingest"])
        _load(ctx, g)
        out = {route: ctx.local_score_test(5, draw=(SEED, 0, route), prepare=True, sharded=True) for route in (1, 2)}
        out["stats"] = _stats(ctx)
        return out


def _dist_pairs(g, world, S, seed=41):
    """Supplied pairs with every ownership pattern at their head: both rows on rank 0, both elsewhere, split, i == j."""
    own = _owner(g, world)
    on0, off0 = np.flatnonzero(own == 0), np.flatnonzero(own != 0)
    rng = np.random.default_rng(seed)
    pi, pj, ni, nj = (rng.integers(0, g["n"], S).astype(np.int32) for _ in range(4))
    pj[::7] = pi[::7]
    if S >= 4:
        pi[:4], pj[:4] = [on0[0], off0[0], on0[0], off0[-1]], [on0[-1], off0[-1], off0[0], off0[-1]]
        ni[:4], nj[:4] = [off0[0], on0[-1], off0[-1], on0[0]], [on0[0], on0[0], off0[0], on0[0]]
    return pi, pj, ni, nj


DIST_CASES = [("thin", 9), ("odd", 300), ("wide", 300)]


def _make_distances():
    for label, S in DIST_CASES:
        for opt in ("rows", "both", "ingest"):
            @_case(f"dist-{label}-{opt}")
            def case(env, label=label, S=S, opt=opt):
                g = _graph(_thin(env.world) if label == "thin" else label)
                ctx, _ = env.context(options=OPTS[opt])
                _load(ctx, g)
                pi, pj, ni, nj = _dist_pairs(g, env.world, S)
                o = ctx.local_score_test(S, pairs=(pi, pj, ni, nj, np.ones(S)), hi=HI, distances=True, sharded=True)
                return dict(dpos=o["dpos"], dneg=o["dneg"], stats=_stats(ctx))

    @_case("dist-wide-second-chunk-rows")
    def case(env):  # K = max(1024, min(S, 64 MB / (16 d))) = 8192 pairs per exchange at d = 512: pair 8192 is a chunk of its own
        g = _graph("wide")
        ctx, _ = env.context(capacity_doubles=1 << 21, options=OPTS["rows"])
        _load(ctx, g)
        pi, pj, ni, nj = _dist_pairs(g, env.world, 8193)
        o = ctx.local_score_test(8193, pairs=(pi, pj, ni, nj, np.ones(8193)), hi=HI, distances=True, sharded=True)
        return dict(dpos=o["dpos"], dneg=o["dneg"])


# whole runs: (graph, options, method, shard_runsplit, shard_samples, auc_samples, ext hooks + wedges_reduce_scatter)
SCORES = [("odd", "both", "rss", 1, 1, 1001, False), ("odd", "both", "rss2", 2, 2, 1001, False),
          ("odd", "both", "size", 0, 2, 3, False), ("odd", "both", "diameter", 2, 2, 1001, False),
          ("odd", "ingest", "rss", 2, 2, 1001, True), ("odd", "none", "rss", 2, 2, 3, False),
          ("odd_w", "rows", "rss", 1, 2, 1001, False),
          ("odd_dir", "both", "rss", 1, 2, 1001, False), ("odd_dir", "ingest", "rss", 2, 1, 3, True),
          ("wide", "both", "rss", 2, 2, 1001, False), ("wide", "rows", "diameter", 0, 2, 3, True)]
LAND = {"odd": 40, "odd_w": 40, "odd_dir": 40, "wide": 24}


def _score_name(cfg):
    g, opt, method, runsplit, samples, auc, ext = cfg
    return f"score-{g}-{opt}-{method}-runsplit{runsplit}-samples{samples}-auc{auc}" + ("-ext" if ext else "")


def _make_scores():
    for cfg in SCORES:
        @_case(_score_name(cfg))
        def case(env, cfg=cfg):
            gname, opt, method, runsplit, samples, auc, ext = cfg
            g = _graph(gname)
            ctx, coll = env.context(capacity_doubles=1 << 18, ext=ext, options=OPTS[opt] + ((("wedges_reduce_scatter", 1),) if ext else ()))
            _load(ctx, g)
            ctx.set_option("shard_runsplit", runsplit)
            ctx.set_option("shard_samples", samples)
            res = [ctx.score(g["clusters"], LAND[gname], 2, method, directed=g["directed"], seed=5, auc_samples=auc) for _ in range(2)]
            tr = ctx.last_trace
            hi = ctx.last_diameter()[0]
            lm = [np.ascontiguousarray(x) for x in ctx.landmarks_fetch()]
            return dict(res=res, hi=hi, lm=lm, n_alpha=tr["n_alpha"], iters=len(tr["iters"]), stats=_stats(ctx),
                        exchanges=(coll.n_calls, coll.n_gather, coll.n_reduce_scatter))


REFUSALS = [("pair", (3, 5)), ("tiny", (5,))]


def _make_refusals():
    for gname, worlds in REFUSALS:
        for opt in ("rows", "both"):
            @_case(f"refuse_rows-{gname}-{opt}", worlds)
            def case(env, gname=gname, opt=opt):
                from cge.jl_amd import api

                g = _graph(gname)
                ctx, _ = env.context(options=OPTS[opt])
                try:
                    _load(ctx, g)
                    first = "no error"
                except api.CGEError as e:
                    first = (e.code, str(e))
                rows_after = int(ctx.get_stat("rows_resident"))
                # the context goes on: without the option the same upload succeeds and the hook measures pairs on it
                ctx.set_option("shard_rows", 0)
                ctx.set_embedding(g["embedding"])
                pi, pj, ni, nj = (np.arange(g["n"], dtype=np.int32), np.arange(g["n"], dtype=np.int32)[::-1].copy(),
                                  np.zeros(g["n"], np.int32), np.arange(g["n"], dtype=np.int32))
                o = ctx.local_score_test(g["n"], pairs=(pi, pj, ni, nj, np.ones(g["n"])), hi=HI, distances=True, sharded=True)
                return dict(first=first, rows_after=rows_after, dpos=o["dpos"], dneg=o["dneg"])

    @_case("refuse_tally-odd-rows")
    def case(env):
        from cge.jl_amd import api

        g = _graph("odd")
        ctx, _ = env.context(options=OPTS["rows"])
        _load(ctx, g)
        errs = []
        n = g["n"]
        pairs = (np.zeros(4, np.int32), np.ones(4, np.int32), np.zeros(4, np.int32), np.ones(4, np.int32), np.ones(4))
        tally = dict(form=1, N=2, Ta=np.ones(2), v2l=np.zeros(n, np.int32), vw=np.ones(n), lweight=np.ones(2))
        for kw in (dict(draw=(1, 0, 1)), dict(pairs=pairs, dists=(np.zeros(4), np.zeros(4)), tally=tally, sharded=True)):
            try:
                ctx.local_score_test(4, **kw)
                errs.append("no error")
            except api.CGEError as e:
                errs.append((e.code, str(e)))
        return errs


_make_residents()
_make_draws()
_make_prepares()
_make_distances()
_make_scores()
_make_refusals()


def _names(world):
    return [name for name in CASES if world in CASE_WORLDS[name]]


# ---- the worlds and the one-rank context of the parent ---------------------------------------------------------------------------
_RUNS = {}


def _run_world(world):
    _RUNS[world] = rw.run_world(world, __name__, _names(world))
    return _RUNS[world]


@pytest.fixture(scope="module")
def world2():
    return _run_world(2)


@pytest.fixture(scope="module")
def world3():
    return _run_world(3)


@pytest.fixture(scope="module")
def world5():
    return _run_world(5)


@pytest.fixture(scope="module")
def one():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _results(request, world, name):
    assert world in CASE_WORLDS[name]
    return request.getfixturevalue(f"world{world}").results(name)


def _params(pairs):
    return [pytest.param(w, x, id=f"W{w}-{x}") for w, x in pairs]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- residents -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,gname,opt", [pytest.param(w, g, o, id=f"W{w}-{g}-{o}") for g, ws in RES_ROWS for w in ws for o in ("rows", "both")])
def test_sharded_rows_hold_exactly_their_communities(request, world, gname, opt):
    """resident_embedding() of rank r: the rows of the communities dist.community_owner gives to r, in ascending id, bit for bit
    (-0.0 included); C == W (pair at 2, tiny at 3, odd and tiny5 at 5), one rank with a single row (odd at 5)."""
    g = _graph(gname)
    own = _owner(g, world)
    emb = np.ascontiguousarray(g["embedding"])
    out = _results(request, world, f"res_rows-{gname}-{opt}")
    held = 0
    for rank, o in enumerate(out):
        ids = np.flatnonzero(own == rank)
        assert len(ids) > 0
        assert np.array_equal(o["ids"], ids), (rank, o["ids"], ids)
        assert _same_bits(o["rows"], emb[ids]), rank
        assert o["stats"]["rows_resident"] == len(ids) and o["stats"]["rows_total"] == g["n"]
        held += len(ids)
    assert held == g["n"]
    if gname == "odd" and world == 5:
        assert min(len(o["ids"]) for o in out) == 1  # the community of one row has a rank to itself
    if gname == "odd" and world == 2:
        assert max(len(o["ids"]) for o in out) == 200


@pytest.mark.parametrize("world,gname", _params((w, g) for g in RES_INGEST for w in WORLDS))
def test_sharded_ingest_residents(request, world, gname):
    """shard_ingest: every rank ends with EVERY embedding row bit for bit (-0.0 included; n % W != 0 at n = 301 and 5801, n < W at
    few3 on 5 ranks) and with the rows edge_shard(m, r, W) of the edge list where the rule of set_graph shards it -- the whole
    list otherwise, m < W included."""
    from cge.jl_amd.dist import edge_shard

    g = _graph(gname)
    emb = np.ascontiguousarray(g["embedding"])
    out = _results(request, world, f"res_ingest-{gname}")
    assert g["n"] % world != 0 or gname in ("few40", "few3")
    sharded = _edges_are_sharded(g, world)
    assert sharded == (gname == "sparse_w" or (gname == "bigfew" and world == 2))
    held = 0
    for rank, o in enumerate(out):
        assert o["rows"].shape == emb.shape and _same_bits(o["rows"], emb), rank
        assert np.array_equal(o["ids"], np.arange(g["n"]))
        e0, e1 = edge_shard(g["m"], rank, world) if sharded else (0, g["m"])
        assert o["m"] == e1 - e0 == o["stats"]["edges_resident"] and o["stats"]["edges_total"] == g["m"]
        assert e1 > e0  # no rank holds an empty slice: m < W keeps the list whole
        assert np.array_equal(o["src"], g["rows0"][e0:e1, 0]) and np.array_equal(o["dst"], g["rows0"][e0:e1, 1])
        assert o["unit"] == (not g["weighted"])
        if g["weighted"]:
            assert np.array_equal(o["w"], g["eweights"][e0:e1])
        held += e1 - e0
    assert held == (g["m"] if sharded else world * g["m"])


# ---- Draw ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_ref(S):
    g = _graph("dense")
    return (ls.draw_pos(SEED, _dense_stream(S), S, g["m"]),) + ls.draw_neg(SEED, _dense_stream(S), S, g["n"], _dense_pred, False)


@pytest.mark.parametrize("S", DRAW_S)
@pytest.mark.parametrize("world,opt", _params((w, o) for w in WORLDS for o in ("ingest", "both")))
def test_draws_over_a_sharded_edge_list(request, world, opt, S):
    """Both routes of the device sampler on 2.1 million edges split over the ranks: every rank returns the reference's pos (a row
    of the WHOLE list), non-edges, attempt numbers and round count.  Several rounds run at S >= 255 (the todo lists of the flag
    exchange); at every S the LAST sample is rejected in round 0, so at odd S the half-filled last word of the flags decides."""
    out = _results(request, world, f"draw_dense-{opt}")
    pos, ni, nj, att = _dense_ref(S)
    assert att[S - 1] >= 1
    if S >= 255:
        assert att.max() >= 2  # at least three rounds: the second and third read their samples through `todo`
    for rank, o in enumerate(out):
        assert o["stats"]["edges_resident"] < o["stats"]["edges_total"] == _graph("dense")["m"]
        for route in (1, 2):
            r = o[(S, route)]
            assert np.array_equal(r["pos"], pos), (rank, route)
            bad = np.flatnonzero((r["neg_i"] != ni) | (r["neg_j"] != nj) | (r["attempt"] != att))
            assert bad.size == 0, (rank, route, bad[:8], r["neg_i"][bad[:8]], r["neg_j"][bad[:8]], r["attempt"][bad[:8]], att[bad[:8]])
            assert r["rounds"] == att.max() + 1


@pytest.mark.parametrize("world,gname,opt", [pytest.param(w, g, o, id=f"W{w}-{g}-{o}") for w in WORLDS for g in ("odd", "odd_dir")
                                             for o in ("rows", "ingest", "both")])
def test_draw_and_prepare_on_a_small_graph_under_every_option(request, world, gname, opt):
    """n = 301 is below the rule that shards an edge list: under every option the hook's collective opt-in draws and prepares
    with the one-rank kernels on the whole list, on every rank alike, undirected and directed."""
    g = _graph(gname)
    is_edge = _is_edge(g)
    for rank, o in enumerate(_results(request, world, f"draw_prepare-{gname}-{opt}")):
        assert o["stats"]["edges_resident"] == o["stats"]["edges_total"] == g["m"]
        for S in (1, 257):
            pos = ls.draw_pos(SEED, 0, S, g["m"])
            ni, nj, att = ls.draw_neg(SEED, 0, S, g["n"], is_edge, g["directed"])
            exp = ls.prepare(g["rows0"][:, 0], g["rows0"][:, 1], None, pos, None, ni, nj, g["directed"])
            for route in (1, 2):
                r = o[(S, route)]
                assert np.array_equal(r["pos"], pos) and np.array_equal(r["neg_i"], ni) and np.array_equal(r["neg_j"], nj)
                assert np.array_equal(r["attempt"], att) and r["rounds"] == att.max() + 1
                for key, e in zip(("pi", "pj", "ni", "nj", "wts"), exp):
                    assert np.array_equal(r[key], e), (rank, S, route, key)


@pytest.mark.parametrize("world", WORLDS)
def test_two_edges_on_many_vertices(request, world):
    """m = 2 at n = 5801: split one edge a rank at W = 2; at W = 3 and 5 the rule m >= W keeps the list whole (no empty slice).
    Either way the draw and the prepared pairs are the reference's on every rank."""
    g = _graph("bigfew")
    is_edge = _is_edge(g)
    pos = ls.draw_pos(SEED, 0, 5, 2)
    ni, nj, att = ls.draw_neg(SEED, 0, 5, g["n"], is_edge, False)
    exp = ls.prepare(g["rows0"][:, 0], g["rows0"][:, 1], None, pos, None, ni, nj, False)
    assert set(pos.tolist()) == {0, 1}
    for rank, o in enumerate(_results(request, world, "draw_prepare-bigfew-ingest")):
        assert o["stats"]["edges_resident"] == (1 if world == 2 else 2)
        for route in (1, 2):
            assert np.array_equal(o[route]["pos"], pos) and np.array_equal(o[route]["attempt"], att)
            for key, e in zip(("pi", "pj", "ni", "nj", "wts"), exp):
                assert np.array_equal(o[route][key], e), (rank, route, key)


# ---- Prepare -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,gname,opt", [pytest.param(w, g, o, id=f"W{w}-{g}-{o}") for w in WORLDS for g in ("sparse", "sparse_w")
                                             for o in ("ingest", "both")])
def test_prepared_pairs_over_a_sharded_edge_list(request, world, gname, opt):
    """prep_lookup_sharded_kernel + the exchange + prep_store_sharded_kernel: pairs from pos2 where there is one, weights from
    pos, (min, max) when undirected -- for rows that rank 0 alone owns (no other rank is touched), rows of the last rank alone
    (S = 3), and the first and last row of every slice; weighted (dyadic) and unit; all five outputs exactly, on every rank."""
    from cge.jl_amd.dist import edge_shard

    g = _graph(gname)
    src, dst, w = g["rows0"][:, 0], g["rows0"][:, 1], (g["eweights"] if g["weighted"] else None)
    samples = _prepare_samples(g, world)
    lo, hi = edge_shard(g["m"], 0, world)
    assert samples["own0"][0].max() < hi and samples["last"][0].min() >= edge_shard(g["m"], world - 1, world)[0]
    assert np.any(src > dst) and np.any(src < dst)  # rows in both orientations
    out = _results(request, world, f"prepare-{gname}-{opt}")
    for rank, o in enumerate(out):
        assert o["stats"]["edges_resident"] == np.diff(edge_shard(g["m"], rank, world))[0] < g["m"]
        for key, (pos, pos2, ni, nj) in samples.items():
            for directed in (False, True):
                for p2 in (None, pos2):
                    exp = ls.prepare(src, dst, w, pos, p2, ni, nj, directed)
                    got = o[(key, directed, p2 is not None)]
                    for name, e in zip(("pi", "pj", "ni", "nj", "wts"), exp):
                        assert np.array_equal(got[name], e), (rank, key, directed, p2 is not None, name)
        # the chain: drawn and prepared in one call, measured in the next
        c = o["chain"]
        pos = ls.draw_pos(SEED, 3, 257, g["m"])
        ni, nj, att = ls.draw_neg(SEED, 3, 257, g["n"], _is_edge(g), False)
        exp = ls.prepare(src, dst, w, pos, None, ni, nj, False)
        assert np.array_equal(c["pos"], pos) and np.array_equal(c["attempt"], att)
        for name, e in zip(("pi", "pj", "ni", "nj", "wts"), exp):
            assert np.array_equal(c[name], e), (rank, "chain", name)
        X = np.ascontiguousarray(g["embedding"])
        assert _same_bits(c["dpos"], ls.dist(X, exp[0], exp[1], HI)) and _same_bits(c["dneg"], ls.dist(X, exp[2], exp[3], HI)), rank


# ---- Distances -----------------------------------------------------------------------------------------------------------------
def _one_rank_dist(one, g, pairs):
    _load(one, g)
    S = len(pairs[0])
    return one.local_score_test(S, pairs=pairs + (np.ones(S),), hi=HI, distances=True)


def _check_dist(one, g, world, S, out):
    pi, pj, ni, nj = pairs = _dist_pairs(g, world, S)
    own = _owner(g, world)
    X = np.ascontiguousarray(g["embedding"])
    ref = _one_rank_dist(one, g, pairs)
    # the one-rank context meets the criterion of tests/test_gpu_local_score.py: the bits of dist()
    assert _same_bits(ref["dpos"], ls.dist(X, pi, pj, HI)) and _same_bits(ref["dneg"], ls.dist(X, ni, nj, HI))
    # every ownership pattern is among the pairs: both on rank 0, both elsewhere, split, i == j
    a, b = own[np.concatenate((pi, ni))], own[np.concatenate((pj, nj))]
    same = np.concatenate((pi, ni)) == np.concatenate((pj, nj))
    assert np.any((a == 0) & (b == 0)) and np.any((a != 0) & (b != 0)) and np.any((a == 0) != (b == 0)) and np.any(same)
    assert np.count_nonzero(ref["dpos"]) >= S // 2
    for rank, o in enumerate(out):
        for key in ("dpos", "dneg"):
            bad = np.flatnonzero(_bits(o[key]) != _bits(ref[key]))
            assert bad.size == 0, (rank, key, bad[:8], o[key][bad[:8]], ref[key][bad[:8]])


@pytest.mark.parametrize("world,label,opt", [pytest.param(w, g, o, id=f"W{w}-{g}-{o}") for w in WORLDS for g, _ in DIST_CASES
                                             for o in ("rows", "both", "ingest")])
def test_pair_distances_through_the_row_exchange(request, one, world, label, opt):
    """sampled_pair_dist on sharded rows (pair_local_idx, the gather of the owned rows, the exchange, pair_dist_rows_kernel) at
    d = 1, 17 and 512: the bits of the one-rank context, which are dist()'s, on every rank.  (`ingest`: the rows are all-gathered
    into a padded matrix and the one-rank kernel reads it.)"""
    g = _graph(_thin(world) if label == "thin" else label)
    out = _results(request, world, f"dist-{label}-{opt}")
    _check_dist(one, g, world, dict(DIST_CASES)[label], out)
    for rank, o in enumerate(out):
        assert (o["stats"]["rows_resident"] < g["n"]) == (opt != "ingest")


@pytest.mark.parametrize("world", WORLDS)
def test_pair_distances_take_a_second_chunk(request, one, world):
    """S = 8193 at d = 512: 8192 pairs fill the 64 MB of rows of one exchange, the last pair is a chunk of its own."""
    _check_dist(one, _graph("wide"), world, 8193, _results(request, world, "dist-wide-second-chunk-rows"))


# ---- whole runs ----------------------------------------------------------------------------------------------------------------
_SCORE_REF = {}


def _score_ref(one, gname, method, auc):
    key = (gname, method, auc)
    if key not in _SCORE_REF:
        g = _graph(gname)
        _load(one, g)
        try:
            one.set_option("fit_persistent", 1)  # (as the ranks: the launch-per-iteration fit)
            res = one.score(g["clusters"], LAND[gname], 2, method, directed=g["directed"], seed=5, auc_samples=auc)
            tr = one.last_trace
            _SCORE_REF[key] = dict(res=res, hi=one.last_diameter()[0], lm=[np.ascontiguousarray(x) for x in one.landmarks_fetch()],
                                   n_alpha=tr["n_alpha"], iters=len(tr["iters"]))
        finally:
            one.set_option("fit_persistent", 0)
    return _SCORE_REF[key]


@pytest.mark.parametrize("world,cfg", [pytest.param(w, c, id=f"W{w}-{_score_name(c)[6:]}") for w in WORLDS for c in SCORES])
def test_small_whole_runs_reproduce_one_rank(request, one, world, cfg):
    """ctx.score in landmark mode: all four split rules, shard_runsplit 0 / 1 / 2, the tallies split at auc_samples = 1001 and 3,
    with and without the hook's own reduce-scatter / all-gather, directed, weighted, d = 512.  v_to_l, the landmark tables and the
    diameter to the bit; elements 0 and 4 equal, the rest within rtol 1e-12 / atol 1e-14 (the tolerances of
    tests/test_gpu_two_ranks.py); the same bits on every rank; traces of the same length; and twice on one context with the same
    result.  One chunk of the blocked edge list over W ranks: W - 1 ranks take the empty-share branch of the edge scatter."""
    gname, opt, method, runsplit, samples, auc, ext = cfg
    g = _graph(gname)
    ref = _score_ref(one, gname, method, auc)
    assert np.all(np.isfinite(ref["res"]))
    out = _results(request, world, _score_name(cfg))
    held = 0
    for rank, o in enumerate(out):
        st = o["stats"]
        assert st["edges_resident"] == st["edges_total"] == g["m"]  # (n below the rule: a replicated list, split by chunks)
        assert 1 <= st["edge_chunks"] < world  # some rank's share of the chunks is empty
        if "rows" in opt or opt == "both":
            assert st["rows_resident"] == int(np.sum(_owner(g, world) == rank))
            held += st["rows_resident"]
        for k, x in enumerate(o["lm"]):
            assert x.shape == ref["lm"][k].shape and x.tobytes() == ref["lm"][k].tobytes(), (rank, "landmark array", k)
        assert o["hi"] == ref["hi"]
        for res in o["res"]:
            assert res[0] == ref["res"][0] and res[4] == ref["res"][4], (rank, res, ref["res"])
            assert np.allclose(res, ref["res"], rtol=1e-12, atol=1e-14), (rank, res, ref["res"])
        assert _same_bits(o["res"][0], o["res"][1]), (rank, o["res"])  # the second run on the same context
        assert o["n_alpha"] == ref["n_alpha"] and o["iters"] == ref["iters"]
        assert _same_bits(o["res"][1], out[0]["res"][1]), (rank, o["res"][1], out[0]["res"][1])  # every rank holds the same bits
        if ext:
            assert o["exchanges"][2] >= 1  # the landmark-pair matrix went out by row blocks
    if opt in ("rows", "both"):
        assert held == g["n"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,gname,opt", [pytest.param(w, g, o, id=f"W{w}-{g}-{o}") for g, ws in REFUSALS for w in ws for o in ("rows", "both")])
def test_fewer_communities_than_ranks_is_refused_on_every_rank(request, one, world, gname, opt):
    """C < W under shard_rows: EVERY rank returns CGE_E_ARG with the same message (it used to be raised on the rank without a row
    alone, while the others waited in the next all-reduce), nothing stays resident, and the context goes on."""
    g = _graph(gname)
    assert g["C"] < world
    out = _results(request, world, f"refuse_rows-{gname}-{opt}")
    n = g["n"]
    pairs = (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy(), np.zeros(n, np.int32), np.arange(n, dtype=np.int32))
    ref = _one_rank_dist(one, g, pairs)
    for rank, o in enumerate(out):
        assert o["first"] != "no error", rank
        assert o["first"][0] == E_ARG and "fewer communities than ranks" in o["first"][1], (rank, o["first"])
        assert o["first"] == out[0]["first"]  # one code, one message
        assert o["rows_after"] == 0
        assert _same_bits(o["dpos"], ref["dpos"]) and _same_bits(o["dneg"], ref["dneg"])


@pytest.mark.parametrize("world", WORLDS)
def test_the_hook_stays_closed_without_the_flag_and_for_tallies(request, world):
    for rank, errs in enumerate(_results(request, world, "refuse_tally-odd-rows")):
        assert [e[0] for e in errs] == [E_ARG, E_ARG], (rank, errs)
        assert "shard_rows" in errs[0][1] and "sharded = 1" in errs[0][1]
        assert "tally forms" in errs[1][1] and "shard_rows" in errs[1][1]


# ---- the times -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_times_are_reported(request, world):
    """Every case of the world has a record from every rank, and the times are printed (-s): the start-up of the ranks, the cases,
    the whole run."""
    run = request.getfixturevalue(f"world{world}")
    names = _names(world)
    missing = [n for n in names if len(run.records.get(n, {})) != world]
    slow = sorted(run.cases_s.items(), key=lambda kv: -kv[1])[:5]
    print(f"\n  W = {world}: {len(names)} cases; start-up {run.startup_s:.1f} s, cases {sum(run.cases_s.values()):.1f} s, "
          f"whole run {run.total_s:.1f} s; slowest: " + ", ".join(f"{n} {s:.2f} s" for n, s in slow))
    assert not missing, missing
