"""Records tests/golden/eig_bits.npz: SHA-256 digests of what the batched eigen-solver (ctx.group_eig) returns for the stacks
of tests/eig_bits_cases.py.  Run on an MI355X with the library of the commit the bits are pinned to:

    python tests/make_eig_bits_fixture.py <commit the library was built from> [library file under csrc/build] [output file]

One entry per case: the digests of the vectors of the case's base matrices, (n_base, 32) uint8, taken from one launch of the
whole stack of T = 520.  The script refuses to write if a repeated matrix of a stack, a second launch, or the base matrices
launched alone give other bits: the fixture would then pin an accident of placement."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import eig_bits_cases as ebc  # noqa: E402
from cge.jl_amd import api  # noqa: E402


def main():
    commit = sys.argv[1]
    if len(sys.argv) > 2 and sys.argv[2]:
        api._LIB_PATH = os.path.join(os.path.dirname(api._LIB_PATH), sys.argv[2])
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, "golden", "eig_bits.npz")
    ctx = api.Context()
    entries = {}
    for case in ebc.cases():
        A = ebc.stack(case)
        nb = len(ebc.base_matrices(case))
        v = ctx.group_eig(A)
        dg = ebc.digests(v)
        assert np.all(np.isfinite(v)), case
        assert all(np.array_equal(dg[i], dg[i % nb]) for i in range(len(dg))), (case, "a repeated matrix differs")
        assert np.array_equal(ebc.digests(ctx.group_eig(A)), dg), (case, "a second launch differs")
        assert np.array_equal(ebc.digests(ctx.group_eig(A[:nb])), dg[:nb]), (case, "the base matrices alone differ")
        entries[ebc.case_name(case)] = dg[:nb].copy()
        print(ebc.case_name(case), "base matrices", nb, "first digest", bytes(dg[0]).hex()[:16])
    entries["provenance"] = np.array(
        f"ctx.group_eig on one MI355X (gfx950), library built from commit {commit}; stacks of tests/eig_bits_cases.py, T = {ebc.T}")
    np.savez_compressed(out, **entries)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
