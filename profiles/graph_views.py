"""Graph views at the headline shape (n = 10^6, m = 10^7): what it costs to make the graph and the vertex data resident,
today's way and through the views.  Median and minimum of 5 whole calls after a warm-up:

  (a) cge_set_graph of int64 host columns + np.add.at vertex weights on the host + cge_set_vertex_data;
  (b) the host int32 (2, m) view, vertex weights derived;
  (c) the device int64 (2, m) view, unit weights, vertex weights derived (integer counts);
  (d) as (c) with random fp64 weights (the sum in edge order);

the kernels' own event times (ingest GB/s read + written, the two degree forms), and -- with --parent-lib, the parent commit's
libcge_hip.so -- cge_set_graph on int64 host columns by both builds, alternating, 10 repetitions a side.

    python profiles/graph_views.py [--out profiles/r13_graph_views.json] [--parent-lib PATH] [--n 1000000] [--m 10000000]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "all_ms": [round(t, 3) for t in ts]}


def raw_set_graph(lib_path, src, dst, w, m, n):
    """cge_set_graph through a library loaded by path (the parent build and this one side by side in one process)."""
    L = C.CDLL(lib_path)
    h = C.c_void_p()
    assert L.cge_create(C.byref(h), 0, None) == 0
    L.cge_destroy.argtypes = [C.c_void_p]
    L.cge_destroy.restype = None

    def call():
        rc = L.cge_set_graph(h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                             C.c_int64(m), C.c_int64(n))
        assert rc == 0, rc

    return call, (lambda: L.cge_destroy(h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_graph_views.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=10_000_000)
    a = ap.parse_args()
    import torch

    from cge.jl_amd import api

    n, m = a.n, a.m
    rng = np.random.default_rng(13)
    e = rng.integers(1, n + 1, size=(m, 2)).astype(np.int64)
    e[0] = (1, n)
    src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    ones, w = np.ones(m), 3 * rng.random(m) + 0.1
    comm = rng.integers(1, 1001, size=n).astype(np.int64)
    comm[:2] = (1, 1000)
    ei32 = np.ascontiguousarray((e - 1).T.astype(np.int32))
    ei64_dev = torch.from_numpy(np.ascontiguousarray((e - 1).T)).cuda()
    w_dev = torch.from_numpy(w).cuda()
    comm32, comm_dev = (comm - 1).astype(np.int32), torch.from_numpy(comm - 1).cuda()
    ctx = api.Context(0)
    out = {"shape": {"n": n, "m": m}, "whole_calls": {}, "kernels": {}}

    def todays_way():
        ctx.L.cge_set_graph(ctx.h, api._p(src), api._p(dst), api._p(ones), C.c_int64(m), C.c_int64(n))
        vw = np.zeros(n)
        np.add.at(vw, src - 1, ones)
        np.add.at(vw, dst - 1, ones)
        ctx.n = n
        ctx.set_vertex_data(comm, vw)

    def host_view():
        ctx.set_graph_view(ei32, None, n=n, base=0)
        ctx.set_vertex_view(comm32, None, base=0)

    def device_view_unit():
        ctx.set_graph_view(ei64_dev, None, n=n, base=0)
        ctx.set_vertex_view(comm_dev, None, base=0)

    def device_view_weighted():
        ctx.set_graph_view(ei64_dev, w_dev, n=n, base=0)
        ctx.set_vertex_view(comm_dev, None, base=0)

    for key, fn in (("a_set_graph_addat_set_vertex_data", todays_way), ("b_host_int32_view_derived", host_view),
                    ("c_device_int64_view_unit_derived", device_view_unit), ("d_device_int64_view_fp64_weights_derived", device_view_weighted)):
        out["whole_calls"][key] = timed(fn)
        print(key, out["whole_calls"][key], flush=True)
    t0 = time.perf_counter()
    vw = np.zeros(n)
    np.add.at(vw, src - 1, ones)
    np.add.at(vw, dst - 1, ones)
    out["whole_calls"]["a_np_add_at_alone_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    # the kernels' own event times
    ctx.profile_enable(True)
    for key, fn in (("unit", device_view_unit), ("weighted", device_view_weighted)):
        ctx.profile_reset()
        for _ in range(5):
            fn()
        p = ctx.profile()
        k = {name: round(v["total_ms"] / max(v["launches"], 1), 4) for name, v in p.items()}
        byts = m * (2 * 8 + 2 * 4 + (16 if key == "weighted" else 0))  # ids read, ids written, weights read and written
        k["graph_ingest_GBps_read_plus_written"] = round(byts / (k["graph_ingest"] * 1e-3) / 1e9, 1)
        out["kernels"][key] = k
        print(key, k, flush=True)
    ctx.profile_enable(False)
    ctx.close()
    if a.parent_lib:  # cge_set_graph on int64 host columns: the parent build and this one, alternating
        new_call, new_close = raw_set_graph(api.library_path(), src, dst, ones, m, n)
        old_call, old_close = raw_set_graph(a.parent_lib, src, dst, ones, m, n)
        old_call(); new_call()
        old, new = [], []
        for _ in range(10):
            for call, ts in ((old_call, old), (new_call, new)):
                t0 = time.perf_counter()
                call()
                ts.append(round((time.perf_counter() - t0) * 1e3, 3))
        old_close(); new_close()
        bound = max(old) + (max(old) - min(old))
        out["set_graph_int64_host_ab"] = {"parent_ms": old, "this_ms": new, "parent_median_ms": statistics.median(old),
                                          "this_median_ms": statistics.median(new), "bound_ms": round(bound, 3),
                                          "rule": "this median < parent's slowest repetition + parent's spread (max - min)",
                                          "holds": statistics.median(new) < bound}
        print(out["set_graph_int64_host_ab"], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
