#!/usr/bin/env python3
"""cge_compare.py -- score several embeddings of one graph in one call (cge_score_views).

The flags of cge_cli.py, with `-e` given once per embedding; prints one line per embedding: the file name, a tab, and its
result vector as cge_cli.py prints it (the same vector cge_cli.py gives for that file alone).

A `-e` file ending in `.npy` is an (n, d) array, rows in vertex order; it is mapped, not read, and goes to the GPU in its own
dtype (float64 / float32 / float16), so `.npy` files of different dtype and width can be mixed with text embeddings.

    python cge_compare.py -g graph.edgelist -c graph.ecg -e a.embedding -e b.embedding -l 200 --seed 42

As in cge_cli.py, `--louvain-level K` (an extension; the reference has no such flag) chooses the Louvain level when `-c` is absent,
and `--ecg [K]` / `--ecg-wmin x` take ECG communities instead.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def split_embeddings(argv):
    """(argv with the first -e only, [every -e file in order])"""
    files, rest, i = [], [], 0
    while i < len(argv):
        if argv[i] == "-e" and i + 1 < len(argv):
            files.append(argv[i + 1])
            i += 2
            continue
        rest.append(argv[i])
        i += 1
    return (rest + ["-e", files[0]] if files else rest), files


def read_any_embedding(path, n):
    """A `.npy` file as a memory map in its own dtype; every other file as parseargs reads it."""
    import numpy as np
    from cge.jl_amd.args import read_embedding

    if not path.endswith(".npy"):
        return read_embedding(path, n)
    a = np.load(path, mmap_mode="r")
    if a.ndim != 2:
        raise AssertionError(f"{path}: expected an (n, d) array")
    if a.shape[0] != n:
        raise AssertionError("No. rows in embedding and no. vertices in a graph differ.")
    return a


def main(argv=None):
    import numpy as np

    import cge.jl_amd as CGE
    from cge.jl_amd import api
    from cge_cli import julia_vector

    argv = list(sys.argv[1:] if argv is None else argv)
    first_argv, files = split_embeddings(argv)
    (edges, weights, vweights, comm, clusters, embed, verbose, land, forced, method, directed, split, seed,
     samples) = CGE.parseargs(first_argv, embedding_reader=read_any_embedding)
    if not files:
        return 1
    n = embed.shape[0]
    embeddings = [embed] + [read_any_embedding(f, n) for f in files[1:]]  # (text: the library's parallel reader)
    ctx = api.default_context()
    ctx.set_option("exact_packed_directed", 1)  # a directed exact score beyond the resident limit: packed, not refused
    # parseargs' arrays as they are; vweight (src/auxilary.jl:104-110) and the clusters (:199-208) are derived by the library
    # from what is resident -- the same bits and the same clusters as parseargs' own, without its host passes over them
    ctx.set_graph_view(np.asarray(edges), np.asarray(weights, dtype=np.float64), n=n, base=1)
    ctx.set_vertex_view(comm, None, base=1)
    results = ctx.score_views(embeddings, api.FROM_COMM, land, forced, method, directed, split, seed, samples)
    for f, r in zip(files, results):
        print(f"{f}\t{julia_vector(r)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
