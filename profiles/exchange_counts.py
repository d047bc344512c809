"""Exchange counts of a two-rank run through the collective hook (gloo between two processes on one GPU): what the library
issued, by its own count -- `collective_calls` / `collective_bytes` of cge_get_stat -- on both ranks.  Run it on two builds of the
library; a host-side refactor must leave every figure as it was.

    python profiles/exchange_counts.py [--out FILE]

Two cases on the 30 000-vertex graph of tests/test_gpu_two_ranks.py (its inputs and its port helper are reused): `shard_rows`
(with shard_ingest: the unique-row hashes, the landmark tables, the diameter's exchanges, the sampled pairs' rows) and
`wedges_rs` (directed, option wedges_reduce_scatter = 1 and the hook's own all-gather / reduce-scatter: the landmark-pair matrix
by row blocks, the degrees from the blocks, the blocks all-gathered by the fetch).  One JSON line per case."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CASES = {"shard_rows": dict(shard_rows=1, shard_ingest=1, directed=False, ext=False),
         "wedges_rs": dict(wedges_reduce_scatter=1, directed=True, ext=True)}


def _rank(rank, world, port, q, name):
    try:
        import torch
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from cge.jl_amd import api
        from cge.jl_amd.dist import TorchCollectives
        from test_gpu_two_ranks import _graph_rows

        case = CASES[name]
        g = _graph_rows(case)
        ctx = api.Context(0)
        coll = TorchCollectives(ctx, 600 * 600 * 2 + 1024, torch.device("cuda", 0), ext=case["ext"])
        for key in ("shard_ingest", "shard_rows", "wedges_reduce_scatter"):
            ctx.set_option(key, case.get(key, 0))
        ctx.set_inputs(g["edges"], g["eweights"], g["vweights"], g["comm"], g["embedding"])
        ctx.set_option("fit_persistent", 1)  # (two processes cannot both keep a persistent grid resident on one GPU)
        stat = lambda: (ctx.get_stat("collective_calls"), ctx.get_stat("collective_bytes"))
        rec = {"rank": rank, "upload": stat()}
        res = ctx.score(g["clusters"], 600, 2, "rss", directed=case["directed"], seed=5, auc_samples=4000)
        rec["score"] = stat()
        ctx.landmarks_fetch()
        rec["fetch"] = stat()
        rec["result"] = res.tolist()
        rec["hook_calls"] = (coll.n_calls, coll.n_reduce_scatter)
        q.put(rec)
        ctx.close()
    except Exception as e:  # surface the failure in the parent
        import traceback

        q.put({"rank": rank, "error": traceback.format_exc() + repr(e)})
    finally:
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch.multiprocessing as mp
    from test_gpu_two_ranks import _free_port

    lines = []
    for name in CASES:
        mpc = mp.get_context("spawn")
        q = mpc.Queue()
        port = _free_port()
        procs = [mpc.Process(target=_rank, args=(r, 2, port, q, name)) for r in range(2)]
        try:
            for p in procs:
                p.start()
            ranks = sorted((q.get(timeout=300) for _ in procs), key=lambda r: r["rank"])
            for p in procs:
                p.join(60)
        finally:  # a rank that hangs or outlives its report does not stay on the GPU
            for p in procs:
                if p.is_alive():
                    p.kill()
                    p.join()
        lines.append(json.dumps({"case": name, "ranks": ranks}))
        print(lines[-1], flush=True)
        if any("error" in r for r in ranks):  # nothing more is started on the GPU after a failure
            sys.exit(1)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
