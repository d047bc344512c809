"""Directed vect_B on the packed tiles (bvec_tile_dir_packed_kernel + bvec_bins_kernel: form 7 of the testing hook
cge_vect_b_test) against the resident directed tile form (form 4, directed) bit for bit on the same symmetric GD, and against
the per-bin reference of tests/vect_b_dir_ref.py.  One workgroup per stored tile writes its own partials and its mirror tile's,
so a wrong transpose, a wrong base[] position or a stale diagonal tile shows as a wrong bin.  Shapes: vect_b_dir_ref.SHAPES --
a community that straddles a tile boundary in each, ids without members in two, a last tile one vertex wide."""
import numpy as np
import pytest

import vect_b_dir_ref as vr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


def _run(ctx, pr, form):
    r = ctx.vect_b_test(pr["GD"], pr["Ta"], pr["Tb"], pr["comm"], pr["C"], directed=True, form=form)
    assert r["form_ran"] == form
    assert np.all(np.isnan(r["guard"])), ("written past the vector's end", form)
    return r["vectB"]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("shape", sorted(vr.SHAPES))
def test_form_7_is_form_4_bit_for_bit_and_the_definition(ctx, shape, kind):
    N, C = shape
    pr = vr.problem(N, C, kind, 11 * N + C + (kind == "exact"))
    packed, resident = _run(ctx, pr, 7), _run(ctx, pr, 4)
    assert np.array_equal(packed.view(np.uint64), resident.view(np.uint64)), np.flatnonzero(packed != resident)[:8]
    vr.check(pr, packed, f"form 7 {shape} {kind}")
    vr.check(pr, resident, f"form 4 {shape} {kind}")


def test_an_asymmetric_product_is_not_transposed(ctx):
    """Ta = 1, Tb = e_v: bin (a, b) is the sum of GD over the members of a times [v in b] -- a mirror tile written with the
    roles of Ta and Tb swapped gives the transposed vector."""
    pr = vr.problem(321, 12, "exact", 5)
    v = int(np.flatnonzero(pr["comm"] == 12)[0])
    pr = dict(pr, Ta=np.ones(321), Tb=np.eye(321)[v])
    C = pr["C"]
    ref = np.zeros((C, C))
    np.add.at(ref[:, 11], pr["comm"] - 1, pr["GD"][:, v])
    got = _run(ctx, pr, 7)
    assert np.array_equal(got, ref.ravel()) and not np.array_equal(got, ref.T.ravel())


def test_refusals(ctx):
    from cge.jl_amd import api

    pr = vr.problem(256, 2, "exact", 1)
    with pytest.raises(api.CGEError) as e:
        ctx.vect_b_test(pr["GD"], pr["Ta"], pr["Tb"], pr["comm"], pr["C"], directed=False, form=7)
    assert e.value.code == -7 and "form 7 is directed only" in str(e.value), str(e.value)
    small = dict(pr, GD=pr["GD"][:200, :200], Ta=pr["Ta"][:200], Tb=pr["Tb"][:200], comm=pr["comm"][:200])
    with pytest.raises(api.CGEError) as e:
        ctx.vect_b_test(small["GD"], small["Ta"], small["Tb"], small["comm"], 2, directed=True, form=7)
    assert e.value.code == -7 and "256 vertices" in str(e.value), str(e.value)
