"""The batched eigen-solver (d <= 128) keeps its BITS whichever wave of a workgroup plays which role (run with -m gpu on an
MI355X).  group_eig_kernel chooses at entry which physical wave owns which column block and which one runs the tridiagonal
tail, from the SIMDs its waves sit on; waves whose columns are all finished leave the rank-2 update out, and the reflector's
scalars are computed by the waves that need them early and read back by the others.  None of this touches an arithmetic
operation, an operand or a summation order, so nothing but equality is accepted: against SHA-256 digests recorded from the
library before the change (tests/golden/eig_bits.npz, recorded by tests/make_eig_bits_fixture.py; its `provenance` names the
commit), for the stacks of tests/eig_bits_cases.py:

  * widths d = 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128 (both sides of every instance boundary, of the 64-row block
    boundary and of each wave's column block): every family of tests/eig_matrices.py, the recipes of test_group_eig_kernel,
    a diagonal and the zero matrix, in turn, T = 520 (two workgroups per CU and a few that start after others have left);
  * the signed-zero hazard at d = 65, 96, 128: block-diagonal and permuted-diagonal integer matrices (zeros also as -0.0) and
    rank-1 matrices with exact zero rows -- finished columns hold exact zeros while later steps still reflect, and the
    update that finished waves now skip is a - 0 w - 0 u there.

Per case: equal to the fixture under the testing knob test_eig_roles = 0 (by placement), 1 (identity), 2 (reversed), 3 (rotated);
and as prefixes of T = 1, 2, 3, 257, 512, 520, in reversed order, and launched twice in a row: placement, neighbours and
launch size cannot matter."""
import os

import numpy as np
import pytest

import eig_bits_cases as ebc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eig_bits.npz")
CASES = ebc.cases()
IDS = [ebc.case_name(c) for c in CASES]


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _expect(fx, case, index):
    """the recorded digests of the stack's matrices `index` (positions in the stack of T)"""
    base = fx[ebc.case_name(case)]
    assert len(base) == len(ebc.base_matrices(case)), "the fixture was recorded for other stacks"
    return base[np.asarray(index) % len(base)]


def _check(fx, case, v, index, what):
    got, want = ebc.digests(v), _expect(fx, case, index)
    bad = [int(index[i]) for i in range(len(got)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{ebc.case_name(case)} {what}: {len(bad)} matrices differ from the recorded bits, first at stack " \
                    f"positions {bad[:8]} ({fx['provenance']})"


@pytest.mark.gpu
@pytest.mark.parametrize("roles", [0, 1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_role_assignment_gives_the_recorded_bits(ctx, fx, case, roles):
    A = ebc.stack(case)
    ctx.set_option("test_eig_roles", roles)
    try:
        v = ctx.group_eig(A)
    finally:
        ctx.set_option("test_eig_roles", 0)
    _check(fx, case, v, np.arange(len(A)), f"test_eig_roles={roles}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_placement_neighbours_and_launch_size_do_not_matter(ctx, fx, case):
    A = ebc.stack(case)
    T = len(A)
    for t in (1, 2, 3, 257, 512, T):
        _check(fx, case, ctx.group_eig(A[:t]), np.arange(t), f"prefix of {t}")
    _check(fx, case, ctx.group_eig(A[::-1]), np.arange(T)[::-1], "reversed order")
    first, second = ctx.group_eig(A), ctx.group_eig(A)
    _check(fx, case, first, np.arange(T), "first of two launches")
    _check(fx, case, second, np.arange(T), "second of two launches")


def test_the_fixture_covers_the_cases():
    """(no GPU) every case has its digests, one per base matrix, and the provenance names the commit"""
    with np.load(FIXTURE) as z:
        names = set(z.files)
        assert names == set(IDS) | {"provenance"}
        for case in CASES:
            assert z[ebc.case_name(case)].shape == (len(ebc.base_matrices(case)), 32)
        assert "commit c73e922" in str(z["provenance"])
    for d in ebc.HAZARD_WIDTHS:  # the hazard stacks do hold -0.0 and exact zeros outside the blocks
        mats = ebc.base_matrices(("hazard", d))
        assert any(np.signbit(m[m == 0.0]).any() for m in mats) and any((m == 0.0).sum() > d for m in mats)
