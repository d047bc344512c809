"""Directed vect_B (src/divergence.jl:530-538) on a SYMMETRIC power matrix, bin by bin from the definition, and the problems
tests/test_gpu_vect_b_dir_packed.py runs on the device.  No GPU is needed here.

  bin (c_i, c_j) accumulates (Ta_i Tb_j) GD_ij over all ordered pairs, i = j included; GD_ij = GD_ji (the directed model's
  matrix is GD[idx(n, min, max)], :426-432), so the upper tiles hold all of it.

"exact" problems: Ta, Tb in {0, 0.5, 1, 1.5, 2} and GD in {0, 1/4, .., 1}, every product a multiple of 1/16 and every sum exact in
fp64 in any order.  "random" problems against np.longdouble: all terms are non-negative, so a bin of n_k terms summed in any order
satisfies |got - ref| <= (n_k + 3) 2^-53 ref; a bin without terms is exactly +0.0."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53

# community sizes in id order (0 = an id without a member); the vertex order is shuffled.  Every shape has a community that
# straddles a 64-vertex boundary of the community-sorted order.
SHAPES = {
    (256, 2): [100, 156],
    (257, 5): [70, 50, 64, 72, 1],                                   # the last tile is one row / column wide
    (321, 12): [30, 40, 0, 50, 20, 10, 64, 1, 36, 25, 25, 20],       # id 3 (1-based) has no member
    (700, 30): [63, 1, 64, 2, 65, 200, 0] + [13] * 22 + [19],        # the 200 spans four blocks; id 7 has no member
}


def problem(N, C, kind, seed):
    """dict(N, C, comm (ids 1..C), Ta, Tb, GD (symmetric), ref (C * C,), nk (terms per bin; None when exact))."""
    sizes = SHAPES[N, C]
    assert sum(sizes) == N and len(sizes) == C
    rng = np.random.default_rng(seed)
    comm0 = np.repeat(np.arange(C), sizes)
    rng.shuffle(comm0)
    if kind == "exact":
        tv = np.array([0.5, 1.0, 1.5, 2.0, 0.0])
        Ta, Tb = rng.choice(tv, N), rng.choice(tv, N)
        GD = rng.integers(0, 5, (N, N)) / 4.0
    else:
        Ta, Tb = rng.uniform(0.1, 3.0, N), rng.uniform(0.1, 3.0, N)
        GD = rng.random((N, N))
        r = rng.random((N, N))
        GD[r < 0.05] = 0.0
        GD[r > 0.95] = 1.0
    GD = np.triu(GD) + np.triu(GD, 1).T
    flat = comm0[:, None].astype(np.int64) * C + comm0[None, :]
    if kind == "exact":
        P = (Ta[:, None] * Tb[None, :]) * GD
        Z = np.bincount(flat.ravel(), weights=P.ravel(), minlength=C * C)
        assert np.all(Z * 16 == np.round(Z * 16)) and Z.max() * 16 < 2.0 ** 52
        ref, nk = Z, None
    else:
        P = (LD(Ta)[:, None] * LD(Tb)[None, :]) * LD(GD)
        ref = np.zeros(C * C, LD)
        np.add.at(ref, flat.ravel(), P.ravel())
        nk = np.bincount(flat.ravel(), minlength=C * C)
    return dict(N=N, C=C, comm=comm0 + 1, Ta=Ta, Tb=Tb, GD=GD, ref=ref, nk=nk, kind=kind)


def check(pr, got, what):
    """One vector against the reference: exact problems bit for bit, random ones by the derived bound per bin."""
    assert got.shape == pr["ref"].shape, what
    if pr["kind"] == "exact":
        bad = np.flatnonzero(got != pr["ref"])
        assert bad.size == 0, (what, bad[:8], got[bad[:8]], pr["ref"][bad[:8]])
        return
    err = np.abs(LD(got) - pr["ref"])
    bound = (LD(pr["nk"]) + 3) * U * pr["ref"]
    bad = np.flatnonzero(~(err <= bound))  # (~: a NaN fails)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], pr["ref"][bad[:8]], pr["nk"][bad[:8]])
    empty = pr["nk"] == 0
    assert np.all(got[empty] == 0.0) and not np.any(np.signbit(got[empty])), what
