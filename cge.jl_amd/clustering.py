"""Host-side mirror of ``louvain_clust`` (reference: src/clustering.jl:14-68).

The reference shells out to three executables of ``louvain_jll`` through files in /tmp and leaves the LEVEL-1 communities
(``hierarchy -l 1``) in ``<edges file>.ecg``, one "node community" pair per line; ``parseargs`` calls it when the command
line has no ``-c`` (src/auxilary.jl:115-121).  Here the communities come from the device (``cge_louvain``,
csrc/kernels_louvain.hip) and the same file is written.  The reference visits the vertices in an unseeded random order,
so its own runs do not agree with each other; quality (modularity) is what the tests compare.

An extension: ``level=`` asks for another level of the hierarchy that the reference's ``louvain -l -1`` computes and its
``hierarchy -l 1`` throws away (src/clustering.jl:20-24), through ``cge_louvain_levels``.
"""
from __future__ import annotations

import numpy as np


def _write_ecg(path, ids, comm):
    with open(path, "w") as f:
        f.write("\n".join(f"{int(i)} {int(c)}" for i, c in zip(ids, comm)))
        f.write("\n")


def _communities(edges1, weights, ctx, level=1, ecg=None):
    """edges1: (m, 2) 1-based int64; returns comm (n,) for vertices 1..n, 0-based consecutive labels.  `ecg` (a dict of members,
    w_min, seed): ECG communities instead of a Louvain level."""
    from . import api

    level = int(level)
    if level < 1 and level != -1:
        raise ValueError("louvain_clust: level is 1, 2, ... or -1 (the last level)")
    ctx = ctx or api.default_context()
    n = int(edges1.max())
    ctx.set_graph(np.asfortranarray(edges1), np.ones(len(edges1)) if weights is None else weights, n)
    if ecg is not None:
        comm, n_comm, q, _ = ctx.ecg(**ecg)
    elif level == 1:
        comm, n_comm, q, rounds = ctx.louvain()
    else:  # level k, or the last when the hierarchy is shorter (-1: the last)
        comm, n_comm, q, rounds = ctx.louvain_levels(max_levels=max(level, 0))[-1]
    return comm, n_comm, q


def _clust(name, args, ctx, **how):
    from . import api

    if len(args) == 2:
        v_min, path = args
        raw, _ = api.read_table(path, column_major=False)
        e = raw[:, :2].astype(np.int64)
        shift = 1 if float(v_min) == 0.0 else 0
        comm, _, _ = _communities(e + shift, None, ctx, **how)
        n = len(comm)
        _write_ecg(path + ".ecg", np.arange(n) + (1 - shift), comm)
        return path + ".ecg"
    if len(args) == 3:
        filename, edges, weights = args
        comm, _, _ = _communities(np.asarray(edges, dtype=np.int64), np.asarray(weights, dtype=np.float64), ctx, **how)
        _write_ecg(filename + ".ecg", np.arange(len(comm)) + 1, comm)  # the weighted form always drops row 0 (:67)
        return filename + ".ecg"
    raise TypeError(f"{name}(v_min, edges_file) or {name}(filename, edges, weights)")


def louvain_clust(*args, ctx=None, level=1):
    """``louvain_clust(v_min::Float64, edges::String)`` (src/clustering.jl:14-29) or
    ``louvain_clust(filename::String, edges::Array{Int,2}, weights::Array{Float64,1})`` (:42-68).  Writes
    ``<file>.ecg`` with one "vertex community" line per vertex, vertex ids in the edge file's own base (the reference
    drops the phantom vertex 0 of a 1-based file, :25-28).

    ``level`` (keyword only; an extension, the reference always writes level 1): k >= 1 writes level k of the Louvain
    hierarchy, or its last level if it has fewer; -1 writes the last level."""
    return _clust("louvain_clust", args, ctx, level=level)


def ecg_clust(*args, ctx=None, members=16, w_min=0.05, seed=0):
    """An extension: the two call forms of ``louvain_clust`` and the same ``<file>.ecg``, with ECG communities
    (``cge_ecg``: `members` relabelled level-1 passes, edges reweighted by co-membership with the floor `w_min` off the 2-core, the
    last level of the Louvain hierarchy on those weights) -- how the community files the reference ships were made."""
    return _clust("ecg_clust", args, ctx, ecg=dict(members=members, w_min=w_min, seed=seed))
