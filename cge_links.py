#!/usr/bin/env python3
"""cge_links.py -- link prediction under the model a score fits (an extension; the reference prints the score alone).

Takes cge_cli.py's flags (src/auxilary.jl:61-219) and scores the embedding the same way, but keeps the geometric Chung-Lu model
of the best alpha and asks it for predictions:

    python cge_links.py -g graph.edgelist -c graph.ecg -e graph.embedding -l 200 --seed 42 --topk 10

    --which local|global   the alpha whose model is kept: the best local score (element 5, default) or the best divergence (1)
    --topk K               per query vertex, the K (1..64, default 10) most probable vertices it has no edge to
    --queries FILE         the query vertices, one id per line (default: every vertex, in chunks)
    --pairs FILE           instead of top-k lists: the model's probability of the pairs `i j` of FILE, one per line
    --keep-edges           do not leave the query's own neighbours out (the model's nearest candidates: graph reconstruction)
    --rank FILE            instead of top-k lists: the exact filtered rank of the held-out pairs `i j` of FILE among the candidates
                           of i (the graph given with -g is the training graph); excludes --pairs and --queries
    --sample FILE          instead of top-k lists: one random graph drawn from the model (every pair an edge with its probability),
                           written to FILE as `i j` rows sorted by (i, j); excludes --rank, --pairs and --queries
    --sample-seed S        the seed of that draw (default 0)
    --auc                  instead of top-k lists: the exact local score and AUC of the kept model, every edge against every
                           non-edge (what element 5 of the vector estimates from samples); excludes the four above

    --moments FILE         instead of top-k lists: the model summed over EVERY pair (Context.link_moments): per community bin the
                           observed edge mass, the model's expectation, its standard deviation and z, written to FILE as
                           `a b observed expected sd z` rows; --which defaults to global; excludes the five above
    --degrees FILE         with --moments: `v weight expected_out [expected_in]` per vertex (its weight beside the model's
                           expected degree), written to FILE
    --clustering FILE      instead of top-k lists: expected and observed triangles and wedges per vertex (Context.link_triangles;
                           undirected only), written to FILE as `v tri_obs wed_obs tri_exp wed_exp` rows, v 1-based; excludes
                           the six above

stdout: the 7-vector line cge_cli.py prints, then one `i j p` line per prediction, ids in the edge file's own base (0 or 1).
With --rank: one `i j p greater ties cand` line per pair (candidates of i other than j that the model puts above / level with j,
and their number), then one `# ` line with MRR, Hits@K, mean rank and AUC (api.link_metrics).
With --auc: one line `# local_exact=... auc=... pos=... neg=... survivors=...` (Context.link_auc; survivors = the pairs the
filter left to exact evaluation).
With --moments: one line `# global_vertex=... global_sweep=... alpha=... which=...`: the Jensen-Shannon divergence between the
observed bins and the model's bins summed over all vertex pairs, beside element 2 of the vector (in landmark mode that one sums
landmark pairs: the difference is what the landmark approximation costs the global score).
With --clustering: one line `# transitivity_obs=... transitivity_exp=... triangles_obs=... triangles_exp=...` (transitivity = sum of
the triangle column / sum of the wedge column, triangles = sum of the triangle column / 3).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cge_cli import julia_float, julia_vector  # noqa: E402

CHUNK = 16384  # query vertices per call when every vertex is asked


class LinkArgError(Exception):
    pass


def link_args(argv):
    """The flags of this script beside cge_cli.py's: {"which", "topk", "queries", "pairs", "exclude"}, with --sample FILE also
    {"sample", "sample_seed"}, with --auc also {"auc"}.  Needs no GPU."""
    argv = list(argv)

    def value(flag):
        if flag not in argv:
            return None
        i = argv.index(flag)
        if i + 1 >= len(argv) or argv[i + 1].startswith("-"):
            raise LinkArgError(f"{flag} needs a value")
        return argv[i + 1]

    which = value("--which") or ("global" if "--moments" in argv else "local")
    if which not in ("local", "global"):
        raise LinkArgError(f"--which is local or global, not {which}")
    topk = value("--topk")
    try:
        topk = 10 if topk is None else int(topk)
    except ValueError:
        raise LinkArgError(f"--topk takes a number, not {topk}") from None
    if not 1 <= topk <= 64:
        raise LinkArgError("--topk is 1 .. 64")
    queries, pairs = value("--queries"), value("--pairs")
    if queries is not None and pairs is not None:
        raise LinkArgError("--queries and --pairs exclude each other")
    for flag, fn in (("--queries", queries), ("--pairs", pairs)):
        if fn is not None and not os.path.isfile(fn):
            raise LinkArgError(f"{flag}: {fn} is not a file")
    if which == "local" and "--samples-local" in argv and int(value("--samples-local")) < 1:
        raise LinkArgError("--which local needs --samples-local >= 1")
    out = {"which": which, "topk": topk, "queries": queries, "pairs": pairs, "exclude": "--keep-edges" not in argv}
    if "--sample" in argv:  # (the keys "sample" / "sample_seed" are there only with the flag)
        out["sample"] = value("--sample")
        if out["sample"] is None:
            raise LinkArgError("--sample needs a value")
        for other in ("--rank", "--pairs", "--queries"):
            if other in argv:
                raise LinkArgError(f"--sample and {other} exclude each other")
        seed = value("--sample-seed")
        try:
            out["sample_seed"] = 0 if seed is None else int(seed)
        except ValueError:
            raise LinkArgError(f"--sample-seed takes a number, not {seed}") from None
    elif "--sample-seed" in argv:
        raise LinkArgError("--sample-seed goes with --sample")
    if "--auc" in argv:  # (the key "auc" is there only with the flag)
        for other in ("--sample", "--rank", "--pairs", "--queries"):
            if other in argv:
                raise LinkArgError(f"--auc and {other} exclude each other")
        out["auc"] = True
    if "--moments" in argv:  # (the keys "moments" / "degrees" are there only with the flag)
        out["moments"] = value("--moments")
        if out["moments"] is None:
            raise LinkArgError("--moments needs a value")
        for other in ("--auc", "--sample", "--rank", "--pairs", "--queries"):
            if other in argv:
                raise LinkArgError(f"--moments and {other} exclude each other")
        out["degrees"] = value("--degrees")
    elif "--degrees" in argv:
        raise LinkArgError("--degrees goes with --moments")
    if "--clustering" in argv:  # (the key "clustering" is there only with the flag)
        out["clustering"] = value("--clustering")
        if out["clustering"] is None:
            raise LinkArgError("--clustering needs a value")
        for other in ("--moments", "--auc", "--sample", "--rank", "--pairs", "--queries"):
            if other in argv:
                raise LinkArgError(f"--clustering and {other} exclude each other")
    return out


def rank_args(argv):
    """--rank FILE beside `link_args`' flags: the file's name, or None.  Needs no GPU."""
    argv = list(argv)
    if "--rank" not in argv:
        return None
    i = argv.index("--rank")
    if i + 1 >= len(argv) or argv[i + 1].startswith("-"):
        raise LinkArgError("--rank needs a value")
    fn = argv[i + 1]
    for other in ("--pairs", "--queries"):
        if other in argv:
            raise LinkArgError(f"--rank and {other} exclude each other")
    if not os.path.isfile(fn):
        raise LinkArgError(f"--rank: {fn} is not a file")
    return fn


def metrics_line(mt):
    """The summary line of --rank."""
    return "# " + " ".join(f"{k}={julia_float(float(v))}" for k, v in mt.items())


def auc_line(res, survivors):
    """The line of --auc."""
    return (f"# local_exact={julia_float(res['local_exact'])} auc={julia_float(res['auc'])} pos={res['n_pos']} neg={res['n_neg']} "
            f"survivors={survivors}")


def moments_line(global_vertex, global_sweep, alpha, which):
    """The line of --moments."""
    return (f"# global_vertex={julia_float(float(global_vertex))} global_sweep={julia_float(float(global_sweep))} "
            f"alpha={julia_float(float(alpha))} which={which}")


def clustering_line(t):
    """The line of --clustering (t: api.link_clustering_table's dict)."""
    return (f"# transitivity_obs={julia_float(float(t['transitivity_obs']))} transitivity_exp={julia_float(float(t['transitivity_exp']))} "
            f"triangles_obs={julia_float(float(t['triangles_obs']))} triangles_exp={julia_float(float(t['triangles_exp']))}")


def read_ids(path, columns, base, n):
    """The ids of a query / pair file as 1-based int64 (rows, columns), checked against 1..n; `base` is the edge file's."""
    from cge.jl_amd import api

    raw = api.read_table(path, column_major=False)[0]
    if raw.shape[1] < columns:
        raise LinkArgError(f"{path}: {columns} column(s) of ids expected, {raw.shape[1]} found")
    raw = raw[:, :columns]
    if not np.all(raw == np.floor(raw)):
        raise LinkArgError(f"{path}: ids must be integers")
    ids = raw.astype(np.int64) + (1 - base)
    if ids.size and (ids.min() < 1 or ids.max() > n):
        raise LinkArgError(f"{path}: an id outside the graph's {n} vertices")
    return ids


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        la = link_args(argv)
        rank = rank_args(argv)
    except LinkArgError as e:
        print(f"cge_links: {e}", file=sys.stderr)
        return 1
    import cge.jl_amd as CGE
    from cge.jl_amd import api

    (edges, weights, vweights, comm, clusters, embed, verbose, land, forced, method, directed, split, seed,
     samples) = CGE.parseargs(argv)
    if la.get("clustering") is not None and directed:
        print("cge_links: --clustering is for undirected graphs", file=sys.stderr)
        return 1
    base = int(api.read_table(CGE.args._flag_value(argv, "-g"), column_major=False)[0][:, :2].min())  # the file's own id base
    n = len(vweights)
    ctx = api.default_context()
    ctx.set_option("exact_packed_directed", 1)  # as cge_cli.py
    ctx.set_inputs(edges, weights, vweights, comm, embed)
    try:
        vec, trace = ctx.link_fit(clusters, land, forced, method, directed, split, seed, samples, la["which"])
        sys.stderr.write("." * trace["n_alpha"] + "\n")
        print(julia_vector(vec))
        if len(vec) < 7:  # a directed star graph: the reference's early return leaves no model
            return 0
        out = sys.stdout
        if la.get("auc"):
            res = ctx.link_auc()
            out.write(auc_line(res, ctx.get_stat("link_auc_survivors")) + "\n")
            return 0
        if la.get("moments") is not None:
            mo = ctx.link_moments()
            gv = api.link_divergence(mo.C, mo.B, mo.n_comm, mo.directed, split, ctx=ctx)["global"]
            out.write(moments_line(gv, vec[1], ctx.link_model()["alpha"], la["which"]) + "\n")
            with open(la["moments"], "w") as f:
                for a, b, obs, exp, sd, z in api.link_bins_table(mo.B, mo.V, mo.C, mo.n_comm, mo.directed):
                    f.write(f"{a} {b} {julia_float(obs)} {julia_float(exp)} {julia_float(sd)} {julia_float(z)}\n")
            if la.get("degrees") is not None:
                vw = np.asarray(vweights, dtype=np.float64).ravel()
                with open(la["degrees"], "w") as f:
                    for v in range(n):
                        tail = f" {julia_float(float(mo.deg_in[v]))}" if mo.directed else ""
                        f.write(f"{v + base} {julia_float(float(vw[v]))} {julia_float(float(mo.deg_out[v]))}{tail}\n")
            return 0
        if la.get("clustering") is not None:
            t = api.link_clustering_table(*ctx.link_triangles())
            out.write(clustering_line(t) + "\n")
            with open(la["clustering"], "w") as f:
                for v in range(n):
                    f.write(f"{v + 1} {t['tri_obs'][v]} {t['wed_obs'][v]} {julia_float(float(t['tri_exp'][v]))} "
                            f"{julia_float(float(t['wed_exp'][v]))}\n")
            return 0
        if la.get("sample") is not None:
            si, sj, _, _ = ctx.link_sample(la["sample_seed"], 0)
            with open(la["sample"], "w") as f:
                f.write("".join(f"{i - 1 + base} {j - 1 + base}\n" for i, j in zip(si.tolist(), sj.tolist())))
            return 0
        if rank is not None:
            ij = read_ids(rank, 2, base, n)
            if len(ij) == 0:
                return 0
            if (ij[:, 0] == ij[:, 1]).any():
                raise LinkArgError(f"{rank}: a pair (i, i): a vertex is not its own candidate")
            g, t, cand, p = ctx.link_rank(ij[:, 0], ij[:, 1], la["exclude"])
            for q, (i, j) in enumerate(ij):
                out.write(f"{i - 1 + base} {j - 1 + base} {julia_float(float(p[q]))} {g[q]} {t[q]} {cand[q]}\n")
            out.write(metrics_line(api.link_metrics(g, t, cand)) + "\n")
            return 0
        if la["pairs"] is not None:
            ij = read_ids(la["pairs"], 2, base, n)
            p = ctx.link_prob(ij[:, 0], ij[:, 1]) if len(ij) else np.zeros(0)
            for (i, j), v in zip(ij, p):
                out.write(f"{i - 1 + base} {j - 1 + base} {julia_float(float(v))}\n")
            return 0
        q = read_ids(la["queries"], 1, base, n)[:, 0] if la["queries"] is not None else np.arange(1, n + 1, dtype=np.int64)
        for q0 in range(0, len(q), CHUNK):
            part = q[q0:q0 + CHUNK]
            jj, pp, cnt = ctx.link_topk(part, la["topk"], la["exclude"])
            for r, i in enumerate(part):
                for t in range(int(cnt[r])):
                    out.write(f"{i - 1 + base} {jj[r, t] - 1 + base} {julia_float(float(pp[r, t]))}\n")
    except LinkArgError as e:
        print(f"cge_links: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
