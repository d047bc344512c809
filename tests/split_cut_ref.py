"""Long-double reference, a-priori error bounds and seeded inputs for the cut stage of a landmark split -- the rule's
one-dimensional cut on given projections z, the children's member lists in the rule's order, their values and means -- as the hook
cge_group_cut_test returns them (tests/test_gpu_split_cut.py; tests/test_split_cut_ref.py checks this module itself on the CPU).
Written from the rules, one group at a time:

size / diameter   cut = median of z (odd k: the middle value; even k: a / 2 + b / 2 of the two middle values, in fp64) or
    (min + max) / 2 in fp64.  Rows in their own order: z == cut joins low if low is strictly shorter than high at that moment,
    else high; z < cut low; anything else (a NaN cut too) high.  Exact decisions: no margin.
rss   seeds = first arg-min and first arg-max of z (the same row: homogeneous).  Rounds on the gray rows: t1 = {z < median of the
    gray z}, t2 = the rest; if sum_c wsse(low + t1) < sum_c wsse(high + t2) low absorbs t1 (t1 empty: stop), else high absorbs t2
    (t2 empty: stop); gray empty: done.  A leftover gray set goes low if max(f(low + gray), f(high)) < max(f(low), f(high + gray)),
    else high.  A list = the seed, then every absorbed batch in ascending original index.
rss2  stable ascending order p of z; from both ends one row per step joins the side whose sum_c wsse is strictly smaller (equal:
    high); then the boundary moves down while the larger of the two sums strictly decreases, and up only if it never moved down.
    low = p[0..lo], high = p[hi..k) in sorted order.
wsse = ss - s^2 / ws per column of the triple (sum w x^2, sum w x, sum w); f = its sum over the columns; a child's value is -f of
its rows, its mean s / ws.

Error bounds (u = 2^-53, gamma_n = n u / (1 - n u), k = rows of the GROUP, d columns).  The device may form the triple of a set as
a difference of two running sums over the group in any order (the sorted form of rss does), so the bound of a set S inside its
group G uses G's magnitudes SS_c = sum_G w x^2, A_c = sum_G w |x|, WS = sum_G w:
    a running sum of m <= k terms, each a product of up to two roundings, errs by at most gamma_(m + 1) times the sum of the
    absolute terms; a difference of two of them plus one more addition: e_ss_c = 2 gamma_(k + 2) SS_c, e_s_c = 2 gamma_(k + 2) A_c,
    e_w = 2 gamma_(k + 2) WS -- all three are 0 where every term is a multiple of 2^-10 and the sums of the absolute terms stay
    below 2^43 (class `integer`): every partial sum is then an fp64 number.  With ws' = ws - e_w > 0 (else no bound: infinite)
    |err s_c^2 / ws| <= (2 |s_c| e_s_c + e_s_c^2) / ws' + (s_c^2 / ws) e_w / ws'
    the product, the division, the subtraction and the sum over d columns in any order: gamma_(d + 4) sum_c (ss_c + s_c^2 / ws)
    bound f(S) = sum_c [e_ss_c + (2 |s_c| e_s_c + e_s_c^2) / ws' + (s_c^2 / ws) e_w / ws'] + gamma_(d + 4) sum_c (ss_c + s_c^2 / ws)
    bound mean_c(S) = (e_s_c + |s_c / ws| e_w) / ws' + u |s_c / ws|
size and diameter form a child's sums directly from its own m rows (the side sums), in some order: their values and means are
held to the child's own magnitudes, e_ss_c = gamma_(m + 1) ss_c, e_s_c = gamma_(m + 1) sum_S w |x|, e_w = gamma_(m + 1) ws.
No measured constant enters.  Every comparison of rss and rss2 is evaluated in long double and its MARGIN recorded: |f1 - f2| over
the sum of the two sides' bounds (for a comparison of two maxima: the larger bound of either pair).  A task is DECIDED when its
smallest margin exceeds 1: fp64 arithmetic in any order then takes the same branches, and the lists must be equal.  size and
diameter are always decided."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
RSS, RSS2, SIZE, DIAMETER = 0, 1, 2, 3
RULES = {"rss": RSS, "rss2": RSS2, "size": SIZE, "diameter": DIAMETER}
OK, E_HOMOGENEOUS, E_EMPTY_CLUSTER, E_ARG = 0, -2, -3, -7
EPS = float(np.finfo(np.float64).eps)

WIDTHS = (1, 2, 5, 63, 64, 65, 128, 129, 256, 257, 512)
CLASSES = ("integer", "separated", "gaussian", "offset", "wide_weights")
Z_CLASSES = ("distinct", "ties_at_cut", "all_equal", "tie_at_max", "tie_at_min", "two_values", "signed_zero")
# task order mixed, not sorted: rss2's 16-row blocks, the 64-way search / rounds of 64 rows, cut_sides' stride, a chunk +- 1 and
# a prefix slot boundary in the second chunk, one LDS piece against two pieces + the rank merge (the batches of d > 5, whose longest
# group has 4097 rows)
LENS = (1025, 3, 64, 4097, 16, 257, 1031, 5, 127, 2049, 65, 1024, 15, 256, 1033, 4, 66, 128, 4096, 17, 63, 1032, 255, 129, 67, 1023)
# d <= 5 only.  The sort form is chosen per BATCH by its longest group: up to 32768 rows LDS pieces of 4096 + the rank merge, beyond
# that two device-wide rocPRIM sorts (long groups on average) or rocPRIM's segmented sort.  In the cell's batch (longest group
# 32769) both go through the device-wide sorts; alone, 32768 is the piece limit (8 pieces); a batch of 32769 and many short
# groups takes the segmented sort (tests/test_gpu_split_cut.py runs all three)
LONG = (32768, 32769)


def gamma(n):
    return LD(n) * U / (1 - LD(n) * U)


def group_lengths(d):
    """The batch's groups in task order; beyond d = 129 the groups stop at 300 rows, the two longest come at d <= 5 only"""
    lens = [min(k, 300) if d > 129 else k for k in LENS]
    return lens[:9] + list(LONG) + lens[9:] if d <= 5 else lens


def make_problem(cls, d, seed=0):
    """(X (n, d), w (n,), ids (R,) int32 in random order, off (T + 1,) int32) of data class `cls` at width d; n = R + 16"""
    rng = np.random.default_rng([seed, d, CLASSES.index(cls)])
    lens = group_lengths(d)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(off[-1]) + 16
    ids = rng.permutation(n)[: off[-1]].astype(np.int32)
    w = rng.integers(1, 41, n).astype(np.float64)
    if cls == "integer":  # sums of w x^2 stay below 2^53: exact in any order
        X = rng.integers(-1000, 1001, (n, d)).astype(np.float64)
        w = 2.0 ** rng.integers(-3, 4, n)
    elif cls == "separated":
        X = rng.standard_normal((n, d)) + 40.0 * rng.integers(0, 2, n)[:, None] * np.sign(rng.standard_normal(d))
    elif cls == "gaussian":
        X = rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, d)
    elif cls == "offset":  # a mean of a few spreads
        X = 5.0 + rng.standard_normal((n, d))
    else:  # wide_weights
        X = rng.standard_normal((n, d)) * rng.uniform(0.2, 3.0, d)
        w = np.exp(rng.uniform(-6.0, 6.0, n))
    return np.ascontiguousarray(X), w, ids, off


def _tie_rows(k, rng, n_extra):
    """the rows where a kernel changes lane, wave, stride or chunk, plus a few random ones; at least two rows stay free"""
    rows = {j for j in (0, 63, 64, 255, 256, 1023, k - 1) if j < k} | set(rng.integers(0, k, n_extra).tolist())
    return np.array(sorted(rows)[: k - 2], dtype=np.int64)


def _around(k, ties, c, rng, scale=1.0):
    """z with the rows `ties` equal to c and the others distinct, as many below c as above (one more above): c is the median"""
    z = np.empty(k)
    free = rng.permutation(np.setdiff1d(np.arange(k), ties))
    nb = len(free) // 2
    z[free[:nb]] = c - scale * (1.0 + rng.permutation(nb))
    z[free[nb:]] = c + scale * (1.0 + rng.permutation(len(free) - nb))
    z[ties] = c
    return z


def make_z(zcls, k, rule, rng):
    """projections of one group of k >= 3 rows, of z class `zcls`, aimed at `rule` (rss and rss2 get the median's)"""
    z = rng.permutation(k).astype(np.float64) - k // 2 + 0.25  # distinct, far from the row order; never an integer
    if zcls in ("ties_at_cut", "signed_zero"):
        zero = zcls == "signed_zero"
        ties = _tie_rows(k, rng, int(rng.integers(1, 5)))  # an even or an odd number of ties
        if rule == DIAMETER:  # min + max = 2 c exactly, the ties at the mid-range
            c = 0.0 if zero else 1.0
            z = z * (0.5 if zero else 1.0)  # inside (min, max), none equal to c
            free = rng.permutation(np.setdiff1d(np.arange(k), ties))
            z[free[0]], z[free[1]] = c - (k + 1.0), c + (k + 1.0)
            z[ties] = c
        elif not zero and k % 2 == 0 and rng.random() < 0.4:
            # even k, the two middle values differ and their half-sum a / 2 + b / 2 rounds onto one of them: that row is ON the cut
            a = 1.0
            b = np.nextafter(a, 2.0)
            z = _around(k, np.array([0, k - 1]), a, rng)  # k / 2 - 1 rows below, k / 2 - 1 above
            z[k - 1] = b
        else:  # the two middle values are the same number: many rows equal to the median
            z = _around(k, ties, 0.0 if zero else 0.75, rng)
        if zero:
            z[ties[1::2]] = -0.0  # -0.0 == +0.0: both are ON a cut at zero, and the sort keeps their order
    elif zcls == "all_equal":
        z[:] = 1.5
    elif zcls == "tie_at_max":
        m = int(np.argmax(z))
        z[(m + 1 + rng.integers(0, k - 1, 1 if k < 6 else 2)) % k] = z[m]
    elif zcls == "tie_at_min":
        m = int(np.argmin(z))
        z[(m + 1 + rng.integers(0, k - 1, 1 if k < 6 else 2)) % k] = z[m]
    elif zcls == "two_values":
        z = np.where(rng.random(k) < 0.5, -1.0, 2.0)
        z[rng.permutation(k)[:2]] = (-1.0, 2.0)
    return z


def z_class_of(task, d, cls):
    """z class of a task: every (length, z class) pair comes up as the widths and data classes go round"""
    return Z_CLASSES[(task + d + 3 * CLASSES.index(cls)) % len(Z_CLASSES)]


def make_projections(cls, d, rule, off, seed=0):
    rng = np.random.default_rng([seed, d, CLASSES.index(cls), rule, 99])
    z = np.empty(int(off[-1]))
    for t in range(len(off) - 1):
        z[off[t]:off[t + 1]] = make_z(z_class_of(t, d, cls), int(off[t + 1] - off[t]), rule, rng)
    return z


class GroupTerms:
    """the rows' terms w x^2, w x, w of one group, the group's magnitudes and the bounds that follow from them.  dtype: long
    double sums, or plain fp64 numpy in ANOTHER order (numpy's pairwise sums; rss2: running sums from the far end).  direct: the
    rows ARE the set and its sums are formed directly, in any order (gamma_(k + 1) in place of 2 gamma_(k + 2))"""

    def __init__(self, X, w, rows, dtype=LD, direct=False):
        x, wl = X[rows].astype(dtype), w[rows].astype(dtype)
        self.k, self.d, self.dtype = x.shape[0], x.shape[1], dtype
        self.t2, self.t1, self.t0 = wl[:, None] * (x * x), wl[:, None] * x, wl
        xl, wL = X[rows].astype(LD), w[rows].astype(LD)
        g = gamma(self.k + 1) if direct else 2 * gamma(self.k + 2)
        a2, a1, a0 = wL[:, None] * xl * xl, wL[:, None] * np.abs(xl), wL
        if all((a * 1024 == np.rint(a * 1024)).all() and a.sum(0).max() * 1024 < 2.0 ** 53 for a in (a2, a1, a0)):
            g = LD(0)  # every term is a multiple of 2^-10 and every partial sum stays below 2^43: exact in fp64, in any order
        self.e_ss, self.e_s, self.e_w = g * a2.sum(0), g * a1.sum(0), g * a0.sum()

    def triple(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return self.t2[idx].sum(0), self.t1[idx].sum(0), self.t0[idx].sum()

    def f(self, tr):
        """(sum_c wsse, its bound) of a triple; leading axes allowed: ss, s (..., d), ws (...)"""
        ss, s1, ws = tr
        ws_ = np.asarray(ws)[..., None]
        with np.errstate(all="ignore"):
            q = s1 * s1 / ws_
            val = (ss - q).sum(-1)
            sL, qL, wsL = np.asarray(s1, dtype=LD), np.asarray(q, dtype=LD), np.asarray(ws_, dtype=LD)
            wp = wsL - self.e_w
            b = (self.e_ss + (2 * np.abs(sL) * self.e_s + self.e_s ** 2) / wp + qL * self.e_w / wp).sum(-1) \
                + gamma(self.d + 4) * (np.asarray(ss, dtype=LD) + qL).sum(-1)
            b = np.where((wp > 0).all(-1) & np.isfinite(b), b, np.inf)
        return val, b

    def mean(self, tr):
        ss, s1, ws = tr
        with np.errstate(all="ignore"):
            m = s1 / ws
            mL, wp = np.asarray(m, dtype=LD), LD(ws) - self.e_w
            b = (self.e_s + np.abs(mL) * self.e_w) / wp + U * np.abs(mL)
            b = np.where((wp > 0) & np.isfinite(b), b, np.inf)
        return m, b


class Margin:
    def __init__(self):
        self.least = np.inf

    def less(self, a, ba, b, bb):
        """a < b, with the margin of that comparison noted"""
        den = LD(ba) + LD(bb)
        diff = abs(LD(a) - LD(b))
        m = float(diff / den) if den > 0 and np.isfinite(den) else (np.inf if den == 0 and diff > 0 else 0.0)
        self.least = min(self.least, m)
        return a < b


def cut_rule(z, median, tie_le=False, upper_median=False):
    """size (median) / diameter: (low, high, a row sits on the cut).  tie_le / upper_median: seeded mistakes"""
    z = np.asarray(z, dtype=np.float64)
    k = len(z)
    if np.isnan(z).any():
        cut = np.nan
    elif median:
        zs = np.sort(z)
        cut = zs[k // 2] if (k & 1) or upper_median else zs[k // 2 - 1] / 2.0 + zs[k // 2] / 2.0
    else:
        cut = (z.min() + z.max()) / 2.0
    low, high = [], []
    for j in range(k):
        if z[j] == cut:
            (low if (len(low) <= len(high) if tie_le else len(low) < len(high)) else high).append(j)
        elif z[j] < cut:
            low.append(j)
        else:
            high.append(j)
    return low, high, bool((z == cut).any())


def _median(v):
    vs = np.sort(v)
    n = len(vs)
    return vs[n // 2] if n & 1 else vs[n // 2 - 1] / 2.0 + vs[n // 2] / 2.0


def rss_rule(G, z, mg, equal_goes_low=False):
    """(rc, low, high); equal_goes_low: the seeded mistake: equal sums let low absorb t1"""
    z = np.asarray(z, dtype=np.float64)
    k = len(z)
    imin, imax = int(np.argmin(z)), int(np.argmax(z))
    if imin == imax:
        return E_HOMOGENEOUS, [], []
    low, high = [imin], [imax]
    gray = np.array([j for j in range(k) if j != imin and j != imax], dtype=np.int64)
    add = lambda a, b: (a[0] + b[0], a[1] + b[1], a[2] + b[2])
    rl, rh = G.triple(low), G.triple(high)
    while len(gray):
        below = z[gray] < _median(z[gray])
        t1, t2 = gray[below], gray[~below]
        c1, c2 = add(rl, G.triple(t1)), add(rh, G.triple(t2))
        (f1, b1), (f2, b2) = G.f(c1), G.f(c2)
        first = (not mg.less(f2, b2, f1, b1)) if equal_goes_low else mg.less(f1, b1, f2, b2)
        if first:
            if not len(t1):
                break
            low += t1.tolist()
            rl, gray = c1, t2
        else:
            if not len(t2):
                break
            high += t2.tolist()
            rh, gray = c2, t1
    if len(gray):
        tg = G.triple(gray)
        (a1, ba1), (a2, ba2) = G.f(add(rl, tg)), G.f(rh)
        (c1, bc1), (c2, bc2) = G.f(rl), G.f(add(rh, tg))
        if mg.less(max(a1, a2), max(ba1, ba2), max(c1, c2), max(bc1, bc2)):
            low += gray.tolist()
        else:
            high += gray.tolist()
    return OK, low, high


def rss2_rule(G, z, mg):
    z = np.asarray(z, dtype=np.float64)
    k = len(z)
    p = np.argsort(z, kind="stable")
    t2, t1, t0 = G.t2[p], G.t1[p], G.t0[p]
    if G.dtype == LD:
        pre = (np.cumsum(t2, 0), np.cumsum(t1, 0), np.cumsum(t0))
        suf = (np.cumsum(t2[::-1], 0)[::-1], np.cumsum(t1[::-1], 0)[::-1], np.cumsum(t0[::-1])[::-1])
    else:  # another order: the prefixes as the total less the running sum from the far end, and the other way round
        suf = (np.cumsum(t2[::-1], 0)[::-1], np.cumsum(t1[::-1], 0)[::-1], np.cumsum(t0[::-1])[::-1])
        fwd = (np.cumsum(t2, 0), np.cumsum(t1, 0), np.cumsum(t0))
        z2, z1 = np.zeros((1, G.d)), np.zeros(1)
        pre = tuple(a[0] - np.concatenate([b[1:], zz]) for a, b, zz in zip(suf, suf, (z2, z2, z1)))
        suf = tuple(a[-1] - np.concatenate([zz, a[:-1]]) for a, zz in zip(fwd, (z2, z2, z1)))
    FL, BL = G.f(pre)  # ranks 0..i
    FH, BH = G.f(suf)  # ranks j..k-1
    def run(lo, hi, mg):
        while lo + 1 < hi:
            if mg.less(FL[lo], BL[lo], FH[hi], BH[hi]):
                lo += 1
            else:
                hi -= 1
        moved = False
        while lo > 0:
            if mg.less(max(FL[lo - 1], FH[lo]), max(BL[lo - 1], BH[lo]), max(FL[lo], FH[hi]), max(BL[lo], BH[hi])):
                moved = True
                lo, hi = lo - 1, hi - 1
            else:
                break
        if not moved:
            while hi < k - 1:
                if mg.less(max(FL[hi], FH[hi + 1]), max(BL[hi], BH[hi + 1]), max(FL[lo], FH[hi]), max(BL[lo], BH[hi])):
                    lo, hi = lo + 1, hi + 1
                else:
                    break
        return lo, hi

    # The first step compares the sums of two single rows: both are zero in exact arithmetic (the row goes high), and in fp64
    # both are the rounding residue of w x^2 - (w x)^2 / w, which no bound can order.  Both outcomes are followed: the task is
    # decided when they meet in the same boundary with every later margin above 1.
    m_high, m_low = Margin(), Margin()
    (lo, hi), other = run(0, k - 2, m_high), run(1, k - 1, m_low)
    mg.least = min(m_high.least, m_low.least) if other == (lo, hi) else 0.0
    return OK, p[:lo + 1].tolist(), p[hi:].tolist()


def split_group(X, w, rows, z, rule, dtype=LD, **mistake):
    """One group by `rule`: a dict rc, low, high (positions inside the group, in the rule's order), margin (the least of the
    task; inf for the exact rules), tie (size / diameter: a row on the cut)"""
    mg = Margin()
    tie = False
    if rule in (SIZE, DIAMETER):
        low, high, tie = cut_rule(z, rule == SIZE, **mistake)
        rc = OK
    else:
        G = GroupTerms(X, w, rows, dtype)
        rc, low, high = rss_rule(G, z, mg, **mistake) if rule == RSS else rss2_rule(G, z, mg)
    if rc == OK and (not low or not high):
        rc = E_EMPTY_CLUSTER
    return {"rc": rc, "low": low, "high": high, "margin": mg.least, "tie": tie}


def child_stats(X, w, rows, child, dtype=LD, direct=False):
    """(value, value bound, mean (d,), mean bound (d,)) of the child at positions `child` of the group `rows`.  A one-row child
    has the value DBL_EPSILON, exactly.  direct: the bounds of sums over the child's own rows (size, diameter)"""
    child = np.asarray(child, dtype=np.int64)
    G = GroupTerms(X, w, rows[child], dtype, direct=True) if direct else GroupTerms(X, w, rows, dtype)
    tr = G.triple(np.arange(len(child)) if direct else child)
    f, bf = G.f(tr)
    m, bm = G.mean(tr)
    if len(child) == 1:
        return EPS, 0.0, m, bm
    return -f, bf, m, bm


def worst_ratios(X, w, ids, off, out, t_list=None, direct=False, bounds_out=None):
    """The children the code under test returned (a dict of api.group_cut_test, or one in its layout), judged on their own:
    partition, nlow, values and means against long double.  Returns (worst value error / bound, worst mean error / bound); raises
    AssertionError where a child list is no partition of its group.  direct: the children's sums are formed directly from their
    own rows (size, diameter: the side sums), so the bounds are those of the child alone.  bounds_out (T, 2): receives the value
    bounds"""
    wv = wm = 0.0
    for t in (range(len(off) - 1) if t_list is None else t_list):
        if out["rc"][t] != OK:
            continue
        o, k = int(off[t]), int(off[t + 1] - off[t])
        rows, kids, nl = ids[o:o + k], out["children"][o:o + k], int(out["nlow"][t])
        assert 0 < nl < k, (t, nl, k)
        assert np.array_equal(np.sort(kids), np.sort(rows)), f"task {t}: the children are no partition of the group"
        pos = {int(r): j for j, r in enumerate(rows)}
        for q, (child, got) in enumerate(((kids[:nl], out["vlow"][t]), (kids[nl:], out["vhigh"][t]))):
            val, bv, m, bm = child_stats(X, w, rows, [pos[int(r)] for r in child], direct=direct)
            if bounds_out is not None:
                bounds_out[t, q] = bv
            err = abs(LD(got) - val)
            wv = max(wv, 0.0 if err == 0 else float("inf") if (bv == 0 or not np.isfinite(err)) else float(err / bv))
            err = np.abs(out["cmeans"][t, q].astype(LD) - m)
            with np.errstate(all="ignore"):
                r = np.where(err == 0, 0, np.where(bm == 0, np.inf, err / bm))
            r = float(np.max(np.where(np.isfinite(err), r, np.inf)))
            wm = max(wm, r)
    return wv, wm


def reference_batch(X, w, ids, off, z, rule, dtype=LD, **mistake):
    """every task of a batch: a list of split_group dicts"""
    return [split_group(X, w, ids[off[t]:off[t + 1]], z[off[t]:off[t + 1]], rule, dtype, **mistake) for t in range(len(off) - 1)]


def as_output(X, w, ids, off, refs, dtype=np.float64, sort_children=False, parent_weight=False):
    """a batch of reference results in the layout of api.group_cut_test, values and means in plain fp64 numpy (another summation
    order).  sort_children / parent_weight: seeded mistakes (lists sorted by id; a mean divided by the parent's weight)"""
    T, d = len(off) - 1, X.shape[1]
    out = {"rc": np.zeros(T, np.int32), "nlow": np.zeros(T, np.int32), "children": np.full(int(off[-1]), -1, np.int32),
           "vlow": np.zeros(T), "vhigh": np.zeros(T), "cmeans": np.full((T, 2, d), np.nan), "route": np.zeros(T, np.int32)}
    for t, r in enumerate(refs):
        out["rc"][t] = r["rc"]
        out["nlow"][t] = len(r["low"])
        if r["rc"] != OK:
            continue
        rows = ids[off[t]:off[t + 1]]
        low, high = rows[r["low"]], rows[r["high"]]
        if sort_children:
            low, high = np.sort(low), np.sort(high)
        out["children"][off[t]:off[t + 1]] = np.concatenate([low, high])
        for q, child in enumerate((r["low"], r["high"])):
            x, wt = X[rows[child]], w[rows[child]]
            s1, ws = (wt[:, None] * x).sum(0), wt.sum()
            val = EPS if len(child) == 1 else -float(((wt[:, None] * (x * x)).sum(0) - s1 * s1 / ws).sum())
            out["vlow" if q == 0 else "vhigh"][t] = val
            out["cmeans"][t, q] = s1 / (w[rows].sum() if parent_weight else ws)
    return out


def undecided_share(refs):
    return sum(1 for r in refs if not r["margin"] > 1.0) / max(1, len(refs))


def judge(X, w, ids, off, out, refs, direct=False, bounds_out=None):
    """What the tests of the cut stage demand of a result `out` (the layout of api.group_cut_test) given the reference `refs`.
    Always: the children partition their group with nlow rows low (worst_ratios raises otherwise), the values and means are within
    their bounds of the long-double ones of the RETURNED children.  On decided tasks: rc and the children lists, order included,
    are the reference's.  Returns a dict: value, mean (worst error / bound), rc_differs, lists_differ (task lists), undecided"""
    wv, wm = worst_ratios(X, w, ids, off, out, direct=direct, bounds_out=bounds_out)
    rc_bad, lists_bad, und = [], [], []
    for t, r in enumerate(refs):
        if not r["margin"] > 1.0:
            und.append(t)
            continue
        if int(out["rc"][t]) != r["rc"]:
            rc_bad.append(t)
        elif r["rc"] == OK:
            rows = ids[off[t]:off[t + 1]]
            if not np.array_equal(out["children"][off[t]:off[t + 1]], np.concatenate([rows[r["low"]], rows[r["high"]]])):
                lists_bad.append(t)
    return {"value": wv, "mean": wm, "rc_differs": rc_bad, "lists_differ": lists_bad, "undecided": und}


def passes(verdict):
    return verdict["value"] <= 1.0 and verdict["mean"] <= 1.0 and not verdict["rc_differs"] and not verdict["lists_differ"]


class Cells:
    """(rule name, width, class) -> (X, w, ids, off, z, reference): computed once, shared by the tests of a module, never changed"""

    def __init__(self):
        self.store = {}

    def __call__(self, rule, d, cls):
        if (d, cls) not in self.store:
            self.store[(d, cls)] = make_problem(cls, d)
        X, w, ids, off = self.store[(d, cls)]
        if (rule, d, cls) not in self.store:
            z = make_projections(cls, d, RULES[rule], off)
            self.store[(rule, d, cls)] = (z, reference_batch(X, w, ids, off, z, RULES[rule]))
        return (X, w, ids, off) + self.store[(rule, d, cls)]
