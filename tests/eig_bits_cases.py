"""The stacks of tests/golden/eig_bits.npz: what tests/make_eig_bits_fixture.py records and tests/test_gpu_eig_roles_bits.py
replays.  A case is a width d (or a hazard family at a width) and a stack of T = 520 symmetric matrices: the base matrices of
the case in turn.  520 workgroups are two per CU on a 256-CU part plus a few that start after others have left.

Base matrices of width d: every family of tests/eig_matrices.py, the two recipes of test_group_eig_kernel (a Wishart matrix with
half its columns zero; dyadic entries), a diagonal matrix and the zero matrix.

Hazard cases (d = 65, 96, 128): stacks in which finished columns hold exact zeros while later steps still reflect -- block-
diagonal and permuted-diagonal integer matrices (the zeros outside the blocks also written as -0.0) and rank-1 matrices with
exact zero rows.  A Householder step that updates such a column computes a - 0 w - 0 u, which keeps a -0.0 only for one
sign of the zero product; the solver skips that update in waves whose columns are all finished."""
import hashlib

import numpy as np

import eig_matrices as em

T = 520
WIDTHS = (2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
HAZARD_WIDTHS = (65, 96, 128)
_cache = {}


def _recipes(d):
    """test_group_eig_kernel's matrices: Y'Y with column scales; zero columns; dyadic entries"""
    rng = np.random.default_rng(100 + d)
    mats = []
    for t in range(8):
        k = int(rng.integers(max(2, d // 2), 4 * d + 8))
        Y = rng.normal(size=(k, d)) * rng.uniform(0.2, 3.0, size=d)
        if t % 2 == 0:
            Y[:, : d // 2] = 0.0
        if t % 4 >= 2:
            Y = np.round(Y * 4) / 4
        mats.append(Y.T @ Y)
    return mats


def _int_blocks(rng, d, sizes, neg_zero):
    a = np.full((d, d), -0.0 if neg_zero else 0.0)
    i = 0
    while i < d:
        b = min(int(rng.choice(sizes)), d - i)
        m = rng.integers(-4, 5, size=(b, b)).astype(np.float64)
        m = m + m.T
        m[m == 0.0] = 0.0  # (the blocks' own zeros are +0.0)
        a[i:i + b, i:i + b] = m
        i += b
    return a


def _hazard(d):
    rng = np.random.default_rng([7, d])
    mats = []
    for neg_zero in (False, True):
        mats.append(_int_blocks(rng, d, (1, 2, 5, 17, 33), neg_zero))          # block-diagonal
        mats.append(_int_blocks(rng, d, (31, 32, 33), neg_zero))                # blocks as wide as a wave's columns
        p = rng.permutation(d)
        b = _int_blocks(rng, d, (3, 8, 40), neg_zero)
        mats.append(np.ascontiguousarray(b[np.ix_(p, p)]))                       # the same, rows and columns permuted
        dg = np.full((d, d), -0.0 if neg_zero else 0.0)
        dg[np.arange(d), np.arange(d)] = rng.permutation(np.arange(1.0, d + 1)) * rng.choice([-1.0, 1.0], d)
        mats.append(dg)                                                          # permuted diagonal, both signs
        u = rng.integers(-3, 4, size=d).astype(np.float64)
        u[rng.random(d) < 0.5] = 0.0
        u[d - 1] = 2.0
        r1 = np.outer(u, u)
        r1[r1 == 0.0] = -0.0 if neg_zero else 0.0
        mats.append(r1)                                                          # rank 1 with exact zero rows
    return mats


def base_matrices(case):
    """The base matrices of a case: ("w", d) or ("hazard", d)."""
    if case not in _cache:
        kind, d = case
        if kind == "w":
            mats = [em.family_matrix(name, d) for name in em.FAMILIES] + _recipes(d)
            mats += [np.diag(np.arange(1.0, d + 1)), np.zeros((d, d))]
        else:
            mats = _hazard(d)
        for m in mats:
            assert m.shape == (d, d) and np.array_equal(m, m.T) and np.all(np.isfinite(m))
        _cache[case] = [np.ascontiguousarray(m, dtype=np.float64) for m in mats]
    return _cache[case]


def stack(case):
    """(T, d, d): the base matrices in turn; read-only (shared by the tests)"""
    key = ("stack",) + case
    if key not in _cache:
        base = base_matrices(case)
        s = np.stack([base[i % len(base)] for i in range(T)])
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def cases():
    return [("w", d) for d in WIDTHS] + [("hazard", d) for d in HAZARD_WIDTHS]


def case_name(case):
    return f"{case[0]}{case[1]}"


def digests(v):
    """(T, 32) uint8: SHA-256 of every returned vector's bytes"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    return np.stack([np.frombuffer(hashlib.sha256(row.tobytes()).digest(), dtype=np.uint8) for row in v])
