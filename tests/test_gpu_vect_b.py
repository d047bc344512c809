"""vect_B (src/divergence.jl:226-234, :530-538) bin by bin, in every form the sweep computes it by, and the device-side mode
selection of its divergence (run with -m gpu on an MI355X).

The forms go through the testing hook cge_vect_b_test (the sweep's own layout decision, tables and launch wrappers): 1 staged
row bins, 2 plain gather, 3 contiguous rows, 4 tiles + bins, 5 tiles + bins and JS in one launch, 6 the batch's launches over
two problems, 0 what a sweep of the shape picks.  Every expected value is computed here from the definition:

  undirected  bin (min(c_i, c_j), max(c_i, c_j)) accumulates (Ta_i Tb_j) GD_ij over i <= j;
  directed    bin (c_i, c_j) accumulates over all ordered pairs, i = j included.

V1  "exact" inputs (Ta, Tb in {0.5, 1, 1.5, 2}, GD in {0, 1/4, .., 1}): every product is a multiple of 1/16 and every sum is
    exact in fp64 in any order, so every form must give the float64 reference bit for bit;
V2  "random" inputs against np.longdouble: all terms are non-negative, so a bin of n_k terms summed in any order satisfies
    |got - ref| <= (n_k + 3) 2^-53 ref (two roundings per product, at most n_k - 1 additions, one unit for the reference);
    bins without terms are exactly 0.0; forms 1 == 2 and 4 == 5 == 6 bit for bit, as the kernels' comments promise;
V3  which form a sweep picks (exact and landmark mode) and which shapes a forced form refuses;
V4  JS modes 0, 1, 2 selected on the device (k_js; the one-launch forms 5 and 6) against the long double JS(vC, vB, vI, ..).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53


@pytest.fixture(scope="module")
def ctx():
    from cge.jl_amd import api

    c = api.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------
# the shapes: community sizes in id order (0 = an id without a member); the vertex order is shuffled
def _sizes(name):
    if name == "130x1":  # a single bin
        return [130]
    if name == "257x5":  # undirected row 256 starts beyond the first 256 columns; the last tile is one column wide
        return [70, 50, 64, 72, 1]
    if name == "512x8":  # community boundaries exactly on tile edges
        return [64, 64, 128, 64, 64, 32, 32, 64]
    if name == "513x8":  # ... and one vertex in a tile of its own
        return [64, 64, 128, 64, 64, 64, 64, 1]
    if name == "700x17":  # 1, 2, 63, 64, 65; the 200 spans four blocks: its diagonal bin touches more than four tiles
        return [63, 1, 64, 2, 65, 200] + [30] * 10 + [5]
    if name == "1100x600":  # C > 512: ~35 communities per block
        return [2, 2, 2, 2, 2, 1] * 100
    if name == "600x300e":  # odd ids (1-based) empty; block 0 holds 64 singletons = 127 ids: the tiles decline
        return [0, 1] * 100 + [0, 10] * 50
    if name == "640x10e":  # ids 4 and 5 (1-based) empty, accepted by the tiles
        return [64, 100, 60, 0, 0, 96, 64, 128, 64, 64]
    if name == "8192x3":  # the 64 KiB dynamic-LDS boundary of form 1
        return [3000, 2692, 2500]
    if name == "8256x3":  # beyond it
        return [3000, 2756, 2500]
    if name == "300x4":  # form 6's second problem
        return [100, 60, 76, 64]
    raise KeyError(name)


SMALL = ["130x1", "257x5", "512x8", "513x8", "700x17", "1100x600", "600x300e", "640x10e"]


def _tiles_apply(sizes):
    """The tile forms' preconditions, from their statement: N >= 256, C >= 2, at most 64 ids per 64-vertex block of the
    community-sorted order."""
    N, C = sum(sizes), len(sizes)
    sorted_comm = np.repeat(np.arange(C), sizes)
    spans = [sorted_comm[min(N, b + 64) - 1] - sorted_comm[b] + 1 for b in range(0, N, 64)]
    return N >= 256 and C >= 2 and max(spans) <= 64


def _expected_auto(sizes, directed, landmarks):
    """What plan_layout picks with default options: a landmark-mode undirected sweep sums by tiles wherever they apply, an
    exact-mode sweep beyond 8192 vertices too (undirected: with JS in the same launch, form 5; directed: form 4); every other
    sweep of up to 8192 vertices stages whole rows in LDS (form 1) -- also where the tiles decline."""
    N = sum(sizes)
    if _tiles_apply(sizes) and ((landmarks and not directed) or N > 8192):
        return 4 if directed else 5
    assert N <= 8192
    return 1


def _packed(Z, directed):
    """(C, C) sums by ordered community pair -> vect_B's layout."""
    if directed:
        return Z.ravel()
    C = Z.shape[0]
    B = Z + Z.T
    B[np.diag_indices(C)] = np.diag(Z)
    return B[np.triu_indices(C)]  # row-major upper triangle = idx() order


class Problem:
    def __init__(self, name, directed, kind, seed):
        sizes = _sizes(name)
        self.name, self.directed, self.kind, self.sizes = name, directed, kind, sizes
        N, C = sum(sizes), len(sizes)
        self.N, self.C = N, C
        rng = np.random.default_rng(seed)
        comm0 = np.repeat(np.arange(C), sizes)
        rng.shuffle(comm0)
        self.comm = comm0 + 1
        if kind == "exact":
            tv = np.array([0.5, 1.0, 1.5, 2.0] + ([0.0] if directed else []))
            self.Ta = rng.choice(tv, N)
            self.Tb = rng.choice(tv, N) if directed else self.Ta
            if N > 4096:  # integer arithmetic on index grids: no random stream of N^2 values
                i = np.arange(N, dtype=np.int32)
                GD = ((i[:, None] * 7 + i[None, :] * 13 + (i[:, None] ^ i[None, :])) % 5).astype(np.float64)
                GD *= 0.25
            else:
                GD = rng.integers(0, 5, (N, N)) / 4.0
        else:
            self.Ta = rng.uniform(0.1, 3.0, N)
            self.Tb = rng.uniform(0.1, 3.0, N) if directed else self.Ta
            GD = rng.random((N, N))
            r = rng.random((N, N))
            GD[r < 0.05] = 0.0
            GD[r > 0.95] = 1.0
        live = np.ones((N, N), bool) if directed else np.triu(np.ones((N, N), bool))
        # reference
        flat = (comm0[:, None].astype(np.int64) * C + comm0[None, :])
        if kind == "exact":
            P = (self.Ta[:, None] * self.Tb[None, :]) * GD
            if not directed:
                P = np.triu(P)
            if N > 4096:  # onehot . P . onehot^T (every sum exact, so BLAS's order does not matter)
                H = np.zeros((C, N))
                H[comm0, np.arange(N)] = 1.0
                Z = (H @ P) @ H.T
            else:
                Z = np.bincount(flat.ravel(), weights=P.ravel(), minlength=C * C).reshape(C, C)
            assert np.all(Z * 16 == np.round(Z * 16)) and Z.max() * 16 < 2.0 ** 52
            self.ref = _packed(Z, directed)
            self.nk = None
        else:
            P = (LD(self.Ta)[:, None] * LD(self.Tb)[None, :]) * LD(GD)
            Z = np.zeros(C * C, LD)
            np.add.at(Z, flat[live], P[live])
            self.ref = _packed(Z.reshape(C, C), directed)
            cnt = np.bincount(flat[live], minlength=C * C).reshape(C, C)
            self.nk = _packed(cnt, directed)
        del P
        # what the hook gets: the undirected forms must not read below the diagonal
        if directed or N > 4096:
            self.GD = GD
        else:
            self.GD = np.where(live, GD, np.nan)
        ln = self.ref.size
        self.vC = np.floor(rng.random(ln) * 60.0 - 6.0).clip(0.0)  # non-negative, ~10 % exact zeros, independent of vect_B

    def args(self):
        return self.GD, self.Ta, self.Tb, self.comm, self.C

    def check(self, got, what):
        """One vector against the reference: V1 bit for bit, V2 by the derived bound per bin."""
        assert got.shape == self.ref.shape, what
        if self.kind == "exact":
            bad = np.flatnonzero(got != self.ref)
            assert bad.size == 0, (what, self.name, bad[:8], got[bad[:8]], self.ref[bad[:8]])
            return
        err = np.abs(LD(got) - self.ref)
        bound = (LD(self.nk) + 3) * U * self.ref
        bad = np.flatnonzero(~(err <= bound))  # (~: a NaN fails)
        assert bad.size == 0, (what, self.name, bad[:8], got[bad[:8]], self.ref[bad[:8]], self.nk[bad[:8]])
        empty = self.nk == 0
        assert np.all(got[empty] == 0.0) and not np.any(np.signbit(got[empty])), what


@functools.lru_cache(maxsize=2)  # (the tests of a shape follow one another; the 8k problems are 0.5 GB each)
def _problem(name, directed, kind):
    seed = sum(map(ord, name)) * 4 + 2 * directed + (kind == "exact")
    return Problem(name, directed, kind, seed)


# ---------------------------------------------------------------------------------------------------------------
# JS in long double, straight from src/auxilary.jl:34-52
def _diag_mask(C, directed):
    from cge.jl_amd import api

    ln = C * C if directed else C * (C + 1) // 2
    vI = np.zeros(ln, bool)
    if directed:
        vI[:: C + 1] = True
    elif C <= 700:
        vI[[api.idx(C, i, i) - 1 for i in range(1, C + 1)]] = True
    else:  # idx(C, i, i) in closed form (checked against idx() at the ends and in the middle)
        i = np.arange(C, dtype=np.int64)
        pos = C * i - i * (i - 1) // 2
        for q in (1, 2, C // 2, C - 1, C):
            assert pos[q - 1] == api.idx(C, q, q) - 1
        vI[pos] = True
    return vI


def _js_ref(vC, vB, sel):
    n = int(sel.sum())
    if n == 0:
        return LD(0)
    c, b = LD(vC[sel]), LD(vB[sel])
    p, q = (c + 1) / (c.sum() + n), (b + 1) / (b.sum() + n)
    m = (p + q) / 2
    return (np.sum(p * np.log(p / m)) + np.sum(q * np.log(q / m))) / 2


def _js_refs(vC, vB, C, directed):
    vI = _diag_mask(C, directed)
    return [_js_ref(vC, vB, np.ones(vI.size, bool)), _js_ref(vC, vB, vI), _js_ref(vC, vB, ~vI)], vI


def _check_js(js_dev, vC, vB, C, directed, what):
    refs, vI = _js_refs(vC, vB, C, directed)
    for mode, sel_n in ((0, vI.size), (1, int(vI.sum())), (2, int((~vI).sum()))):
        ref = float(refs[mode])
        if sel_n <= 1:  # no bin (the empty sum) or one (p = q = m = 1): exactly zero in the reference, and on the device
            assert ref == 0.0 and js_dev[mode] == 0.0, (what, mode, js_dev[mode])
        else:  # the relative tolerance means something only away from cancellation
            assert ref >= 1e-3, (what, mode, ref)
            assert js_dev[mode] == pytest.approx(ref, rel=1e-12), (what, mode)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------
def _run(ctx, pr, form, n_modes=2, second=None, landmarks=False):
    r = ctx.vect_b_test(*pr.args(), directed=pr.directed, form=form, landmarks=landmarks, vC=pr.vC, n_modes=n_modes,
                        second=None if second is None else second.args() + (second.vC,))
    assert np.all(np.isnan(r["guard"])), ("written past the vector's end", pr.name, form)
    if second is not None:
        assert np.all(np.isnan(r["second_guard"])), ("written past the second vector's end", pr.name, form)
    return r


def _refused(ctx, pr, form, second=None):
    from cge.jl_amd import api

    with pytest.raises(api.CGEError) as e:
        _run(ctx, pr, form, second=second)
    assert e.value.code == -7 and "vect_b_test" in str(e.value), (pr.name, form, str(e.value))


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("name", SMALL)
def test_every_form_against_the_definition(ctx, name, directed, kind):
    """V1 / V2 / V3 and the JS of the vectors on the small shapes: every form that applies gives the reference's bins, every form
    that does not apply refuses, auto picks what plan_layout's rules say."""
    pr = _problem(name, directed, kind)
    tiles = _tiles_apply(pr.sizes)
    second = _problem("300x4", directed, kind) if pr.C > 4 else None
    got = {}
    for form in (1, 2, 3):  # (3: forced, the relabelled graph of `exact_relabel` below its 8192 vertices)
        r = _run(ctx, pr, form)
        assert r["form_ran"] == form
        pr.check(r["vectB"], f"form {form}")
        got[form] = r
    assert _same_bits(got[1]["vectB"], got[2]["vectB"])  # the staged rows add what the gather adds, in its order
    for form in (4, 5, 6):
        if not tiles or (directed and form > 4) or (form == 6 and second is None):
            if form < 6 or second is not None:
                _refused(ctx, pr, form, second if form == 6 else None)
            continue
        r = _run(ctx, pr, form, second=second if form == 6 else None)
        assert r["form_ran"] == form
        pr.check(r["vectB"], f"form {form}")
        got[form] = r
    for form in (5, 6):  # the bins of the one-launch and the batch kernels are bvec_bins_kernel's additions
        if form in got:
            assert _same_bits(got[form]["vectB"], got[4]["vectB"]), form
    if 6 in got:  # the smaller problem of the shared launch: complete (the grid is sized by the larger C) and right
        second.check(got[6]["second_vectB"], "form 6, second problem")
        alone = _run(ctx, second, 4)
        assert _same_bits(got[6]["second_vectB"], alone["vectB"])
    # auto, exact and landmark mode
    for landmarks in (False, True):
        r = _run(ctx, pr, 0, landmarks=landmarks)
        assert r["form_ran"] == _expected_auto(pr.sizes, directed, landmarks), (name, landmarks, r["form_ran"])
        pr.check(r["vectB"], f"auto, landmarks={landmarks}")
    # V4 on these vectors: k_js over each form's vector; the fused launches give k_js's bits
    for form, r in got.items():
        _check_js(r["js_dev"], pr.vC, r["vectB"], pr.C, directed, (name, form))
    for form in (5, 6):
        if form not in got:
            continue
        r2 = got[form]  # n_modes = 2: internal, external
        assert _same_bits(r2["js_fused"], r2["js_dev"][1:3]), (form, r2["js_fused"], r2["js_dev"])
        r1 = _run(ctx, pr, form, n_modes=1, second=second if form == 6 else None)
        assert _same_bits(r1["js_fused"], r1["js_dev"][0:1]), (form, r1["js_fused"], r1["js_dev"])
        assert _same_bits(r1["vectB"], r2["vectB"])
        if form == 6:
            _check_js(r2["second_js_dev"], second.vC, r2["second_vectB"], second.C, False, (name, "second"))
            assert _same_bits(r2["second_js_fused"], r2["second_js_dev"][1:3])
            assert _same_bits(r1["second_js_fused"], r1["second_js_dev"][0:1])


@pytest.mark.parametrize("form", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["8192x3", "8256x3"])
def test_the_lds_boundary_of_the_staged_rows(ctx, name, form):
    """N = 8192: the last size whose row fits the 64 KiB of dynamic LDS (auto: form 1).  N = 8256: form 1 refuses, auto takes the
    tiles, form 3 is what `N >= 64 C` picks where the tiles are declined.  Exact inputs: bit for bit."""
    pr = _problem(name, False, "exact")
    if form == 1 and pr.N > 8192:
        _refused(ctx, pr, 1)
        return
    r = _run(ctx, pr, form)
    assert r["form_ran"] == (form if form else _expected_auto(pr.sizes, False, False))
    pr.check(r["vectB"], f"form {form}")
    _check_js(r["js_dev"], pr.vC, r["vectB"], pr.C, False, (name, form))
    if r["form_ran"] == 5:
        assert _same_bits(r["js_fused"], r["js_dev"][1:3])


# ---------------------------------------------------------------------------------------------------------------
# V4 on stand-alone vectors: lengths that are no multiple of 256, C up to 3000 (4.5 M packed bins, 9 M directed)
@pytest.mark.parametrize("directed", [False, True], ids=["undirected", "directed"])
@pytest.mark.parametrize("C", [1, 2, 3, 64, 700, 3000])
def test_js_modes_selected_on_the_device(ctx, C, directed):
    rng = np.random.default_rng(1000 + 2 * C + directed)
    ln = C * C if directed else C * (C + 1) // 2
    vC = np.floor(rng.random(ln) * 60.0 - 6.0).clip(0.0)  # exact zeros among them
    vB = rng.random(ln) * 40.0
    vB[rng.random(ln) < 0.1] = 0.0
    r = ctx.vect_b_test(None, None, None, None, C, directed=directed, vC=vC, vB=vB)
    _check_js(r["js_dev"], vC, vB, C, directed, (C, directed))
    if C == 1:
        assert r["js_dev"][2] == 0.0 and not np.signbit(r["js_dev"][2])  # mode 2 selects nothing: the reference's empty sum
