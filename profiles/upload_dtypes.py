#!/usr/bin/env python3
"""upload_dtypes.py -- what an embedding upload costs by the form it arrives in (cge_set_embedding_view).

At the headline shape (n = 10^6, d = 128), in one process, each form is uploaded once to warm up and then `--reps` times; the
wall time of a call is stream-synchronised (every upload entry point returns after its last kernel).  The forms:

    f64_F_host_set_embedding   cge_set_embedding of the float64 column-major array (the fp64 host view): the baseline
    f32_C_host                 cge_set_embedding_view, float32 row-major on the host
    f32_F_host                 ... float32 column-major on the host
    bf16_C_host                ... bfloat16 row-major on the host
    f32_C_device               ... float32 row-major in this GPU's memory
    f64_F_device               cge_set_embedding_device, float64 column-major in this GPU's memory
    f64_C_device               ... float64 row-major (the form bench.py uploads)

Per form: median / min milliseconds, the bytes that crossed the link and their rate over the whole call, and -- from a separate,
event-timed repetition -- the widening kernels' own time and the bytes they read + wrote per second (the copy ceiling of the chip
is 6.3 TB/s).  The call's tail (allocation of the resident matrix, its column means) is common to all forms.  One JSON document
on stdout.

    python profiles/upload_dtypes.py [--n 1000000] [--d 128] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from cge.jl_amd import api

    n, d = args.n, args.d
    rng = np.random.default_rng(1)
    x32 = rng.standard_normal((n, d), dtype=np.float32)
    x64f = np.asfortranarray(x32.astype(np.float64))
    x32f = np.asfortranarray(x32)
    xb = torch.from_numpy(x32).to(torch.bfloat16)
    x32d = torch.from_numpy(x32).cuda()
    x64fd = torch.from_numpy(x64f.T).cuda()  # (d, n) C-order: the column-major (n, d) matrix
    x64cd = x64fd.t().contiguous()
    torch.cuda.synchronize()
    ctx = api.Context(0)
    ctx.set_graph(np.array([[1, n]], dtype=np.int64), np.ones(1), n)
    forms = [("f64_F_host_set_embedding", lambda: ctx.set_embedding(x64f), 8 * n * d, 8),
             ("f32_C_host", lambda: ctx.set_embedding_view(x32), 4 * n * d, 4),
             ("f32_F_host", lambda: ctx.set_embedding_view(x32f), 4 * n * d, 4),
             ("bf16_C_host", lambda: ctx.set_embedding_view(xb), 2 * n * d, 2),
             ("f64_F_device", lambda: ctx.set_embedding_device(x64fd.data_ptr(), n, d, row_major=False), 0, 8),
             ("f64_C_device", lambda: ctx.set_embedding_device(x64cd.data_ptr(), n, d, row_major=True), 0, 8),
             ("f32_C_device", lambda: ctx.set_embedding_view(x32d), 0, 4)]
    out = {"n": n, "d": d, "reps": args.reps, "forms": {}}
    for name, call, link_bytes, es in forms:
        call()  # warm-up
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_all": [round(v, 3) for v in ms],
               "link_bytes": link_bytes}
        if link_bytes:
            rec["link_GBps_over_call"] = round(link_bytes / (statistics.median(ms) * 1e-3) / 1e9, 2)
        ctx.profile_enable(True)  # one more repetition with the kernels bracketed by events
        ctx.profile_reset()
        call()
        prof = {k: v for k, v in ctx.profile().items() if k.startswith("ingest_") and v["launches"]}
        ctx.profile_enable(False)
        kms = sum(v["total_ms"] for v in prof.values())
        if kms > 0:
            rec["widen_kernels"] = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 4)} for k, v in prof.items()}
            rec["widen_GBps_read_plus_write"] = round((es + 8) * n * d / (kms * 1e-3) / 1e9, 1)
        out["forms"][name] = rec
    got, _ = ctx.resident_embedding()  # (the last form left the widened matrix resident)
    out["last_form_exact"] = bool(np.array_equal(got, x32.astype(np.float64)))
    base = out["forms"]["f64_F_host_set_embedding"]["ms_median"]
    out["speedup_over_f64_baseline"] = {k: round(base / v["ms_median"], 3) for k, v in out["forms"].items()}
    print(json.dumps(out, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
