"""Problems and recorder of tests/golden/split_stats_bits.npz: SHA-256 digests of what the statistics stage of a landmark split
(hook cge_group_stats_test) returns -- cov, vec, z, mean -- recorded from the library of ONE commit, so that a rework of the
covariance and eigen-solver kernels can be held to the same bits (tests/test_gpu_split_stats_bits.py imports the problems
from here: one definition).

    python tests/make_split_stats_bits_fixture.py --commit $(git rev-parse HEAD) [--out tests/golden/split_stats_bits.npz]

needs an MI355X and the built library; the commit it ran on goes into the fixture's `provenance` string.  The fixture holds
digests only (32 bytes per array, and a 2-byte tag per task of the scheduling case), in few arrays: about 10 KB."""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import group_stats_ref as gs  # noqa: E402

KEYS = ("cov", "vec", "z", "mean")
CLASS_WIDTHS = (48, 63, 64, 65, 127, 128)  # partial MFMA tiles, the unpaired loads of odd d, both register forms of the solver
SCHED_WIDTHS = (64, 128)
EDGE_WIDTHS = (2, 3, 64, 65, 128)
SCHED_ROWS = 44000
SCHED_LONG = (1024, 1500, 2049, 2500, 3000)  # one chunk exactly, two, three (2049 = 2 * 1024 + 1), three, three
SCHED_SHORT = 2000


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def task_tags(out, off):
    """(T,) uint16: the first two bytes of the SHA-256 of task t's cov, vec, z and mean together (they name the tasks that differ;
    the digests of the whole arrays are the check)"""
    tags = np.empty(len(off) - 1, dtype=np.uint16)
    for t in range(len(off) - 1):
        h = hashlib.sha256()
        for a in (out["cov"][t], out["vec"][t], out["z"][off[t]:off[t + 1]], out["mean"][t]):
            h.update(np.ascontiguousarray(a).tobytes())
        tags[t] = int.from_bytes(h.digest()[:2], "little")
    return tags


def sched_problem(d):
    """(X (SCHED_ROWS, d), w, ids, off): SCHED_SHORT groups of 1 .. 60 rows (1 + floor(60 u^3), u uniform: 16 rows on average, so
    that they and the long groups fit the table) with the five groups of SCHED_LONG dealt among them, ids a random draw of the
    table's rows.  About 2050 chunks of very unequal length: more half-tile work units than a chip holds at once."""
    rng = np.random.default_rng([7, d])
    lens = np.minimum(1 + np.floor(60.0 * rng.random(SCHED_SHORT) ** 3).astype(np.int64), 60)
    for k, at in zip(SCHED_LONG, (3, 411, 1000, 1777, 2003)):  # near the front, inside, the next to last task
        lens = np.insert(lens, at, k)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert off[-1] <= SCHED_ROWS, off[-1]
    ids = rng.permutation(SCHED_ROWS)[: off[-1]].astype(np.int32)
    X = rng.standard_normal((SCHED_ROWS, d)) * rng.uniform(0.2, 3.0, d) + 2.0 * rng.standard_normal((8, d))[rng.integers(0, 8, SCHED_ROWS)]
    w = rng.integers(1, 41, SCHED_ROWS).astype(np.float64)
    return np.ascontiguousarray(X), w, ids, off


def sched_long_tasks(off):
    lens = np.diff(off)
    return [int(t) for t in np.flatnonzero(lens >= 1024)]


def edge_diagonals(d):
    """The diagonals (small integers k_i^2 * 2 w_i, w_i in {1, 4, 9}: exact square roots) of the exactly diagonal covariances of the
    edge-case groups at width d: mixed, all equal (one eigenvalue d times), with zero entries, largest entry last / first"""
    rng = np.random.default_rng([11, d])
    k = [rng.integers(1, 6, d), np.full(d, 3), rng.integers(0, 4, d), np.arange(d) % 5 + 1, 5 - np.arange(d) % 5]
    k[2][0] = 3  # (never all zero)
    w = [rng.choice([1, 4, 9], d), np.full(d, 4), rng.choice([1, 4, 9], d), np.ones(d, dtype=np.int64), np.full(d, 9)]
    return [(ki.astype(np.int64), wi.astype(np.int64)) for ki, wi in zip(k, w)]


def edge_problem(d):
    """(X, w, ids, off): per group rows +k_i e_i and -k_i e_i of weight w_i for every column i (mean exactly 0, covariance exactly
    diag(2 w_i k_i^2), every product and sum an integer), in shuffled order; a last group of 7 identical rows (the zero matrix)."""
    rng = np.random.default_rng([13, d])
    rows, wts, lens = [], [], []
    for k, wt in edge_diagonals(d):
        R = np.zeros((2 * d, d))
        R[np.arange(d), np.arange(d)] = k
        R[d + np.arange(d), np.arange(d)] = -k
        p = rng.permutation(2 * d)
        rows.append(R[p])
        wts.append(np.concatenate([wt, wt])[p].astype(np.float64))
        lens.append(2 * d)
    rows.append(np.tile(rng.integers(-8, 9, d).astype(np.float64), (7, 1)))  # integers: the mean is the row itself
    wts.append(rng.integers(1, 9, 7).astype(np.float64))
    lens.append(7)
    X, w = np.ascontiguousarray(np.concatenate(rows)), np.concatenate(wts)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return X, w, np.arange(off[-1], dtype=np.int32), off


def sturm_meets_zero(dg):
    """Whether the 64-way multisection of the largest eigenvalue of diag(dg) (off-diagonal exactly 0: q_i = dg_i - x, whatever
    the reciprocal gives) meets q == 0.0 -- the device loop's section points, bracket update and exit test in fp64 numpy."""
    dg = np.asarray(dg, dtype=np.float64)
    gn = np.abs(dg).max()
    tiny = max(gn, 2.2250738585072014e-308) * 2.220446049250313e-16
    lo, hi = dg.min(), dg.max() + tiny
    frac = (np.arange(64, dtype=np.float64) + 1.0) / 65.0
    met = False
    for _ in range(64):
        x = lo + (hi - lo) * frac
        q = dg[None, :] - x[:, None]
        met |= bool((q == 0.0).any())
        full = (q < 0).sum(1) >= len(dg)
        if not full.any():
            nlo, nhi = x[63], hi
        else:
            f = int(np.argmax(full))
            nhi, nlo = x[f], (x[f - 1] if f > 0 else lo)
        if not (nhi > nlo) or (nlo == lo and nhi == hi):
            break
        lo, hi = max(lo, nlo), min(hi, nhi)
    return met


def load(ctx, X, w):
    ctx.set_vertex_data(np.ones(len(w), dtype=np.int64), w)
    ctx.set_embedding(X)


def record(new_ctx):
    """{key: digest or tags} of every problem; new_ctx() opens a context of the library under test (a context keeps the number
    of rows of its first table: one per table size)"""
    fx = {}
    ctx = new_ctx()
    for d in CLASS_WIDTHS:
        for cls in gs.CLASSES:
            X, w, ids, off = gs.make_problem(cls, d)
            load(ctx, X, w)
            out = ctx.group_stats_test(ids, off)
            for k in KEYS:
                fx[f"class/{cls}/{d}/{k}"] = digest(out[k])
    ctx.close()
    ctx = new_ctx()
    for d in SCHED_WIDTHS:
        X, w, ids, off = sched_problem(d)
        load(ctx, X, w)
        out = ctx.group_stats_test(ids, off)
        for k in KEYS:
            fx[f"sched/{d}/{k}"] = digest(out[k])
        fx[f"sched/{d}/task_tags"] = task_tags(out, off)
    ctx.close()
    for d in EDGE_WIDTHS:
        X, w, ids, off = edge_problem(d)
        ctx = new_ctx()
        load(ctx, X, w)
        out = ctx.group_stats_test(ids, off)
        ctx.close()
        for k in KEYS:
            fx[f"edge/{d}/{k}"] = digest(out[k])
    return fx


def save_fixture(path, fx, provenance):
    """digests as ONE (n, 32) array beside their keys (an array per digest costs ten times its bytes in a .npz)"""
    keys = sorted(k for k in fx if not k.endswith("task_tags"))
    tags = {k.replace("/", "_"): fx[k] for k in fx if k.endswith("task_tags")}
    np.savez_compressed(path, keys=np.array(keys), digests=np.stack([fx[k] for k in keys]), provenance=np.array(provenance), **tags)


def load_fixture(path):
    with np.load(path, allow_pickle=False) as f:
        fx = {str(k): dg for k, dg in zip(f["keys"], f["digests"])}
        for d in SCHED_WIDTHS:
            fx[f"sched/{d}/task_tags"] = f[f"sched_{d}_task_tags"]
        fx["provenance"] = str(f["provenance"])
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library is loaded (git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "golden", "split_stats_bits.npz"))
    a = ap.parse_args()
    from cge.jl_amd import api

    fx = record(lambda: api.Context(0))
    again = record(lambda: api.Context(0))
    assert all(np.array_equal(fx[k], again[k]) for k in fx), "two recordings differ"
    save_fixture(a.out, fx, f"recorded on an MI355X (gfx950) from the library built at commit {a.commit}, before the covariance "
                            f"SYRK and the multisection loop were reworked; {len(fx)} entries, recorded twice with equal bits")
    print(f"wrote {a.out}: {len(fx)} entries, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
