"""A plain reference of the local half of the score (elements 5-7 of a score vector, src/divergence.jl:178-213, :485-517) for
tests/test_gpu_local_score.py: Python integers and numpy, nothing of the kernels.

  the sampler   the counter-based stream of the library (a splitmix64 finaliser over (seed, stream, k, attempt, which), a
                multiply-high bounded draw) in 64-bit Python integers; the positive draw, and the non-edge draw as a loop per
                sample over the attempt numbers -- a sample depends on (seed, stream, k, attempt) alone;
  dist()        src/auxilary.jl:14-20: differences, products, an ascending unfused sum in fp64, the root, then / hi;
  the tallies   np.longdouble: pos and neg of every sample (landmark mode and exact mode), the indicator pos > neg, the weights,
                num and den, the relative gap of every sample and the slot of sample k in the two grids of the tally kernels.

Pinned on the CPU by tests/test_local_score_ref.py, which also holds every input condition the GPU tests rely on.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
M64 = (1 << 64) - 1
BLOCKS, WIDE, WIDE_MIN = 64, 16, 65536  # block tallies, the wide grid's blocks per slot, its first sample count


# ---- the counter-based stream ------------------------------------------------------------------------------------------------
def sm64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def ctr_rand(seed, stream, k, attempt, which):
    h = sm64((seed & M64) ^ 0x6A09E667F3BCC909)
    h = sm64(h ^ (((stream & M64) * 0xD1342543DE82EF95 + 1) & M64))
    h = sm64(h ^ ((k * 0x2545F4914F6CDD1D + 2) & M64))
    h = sm64(h ^ ((attempt * 0x9E6C63D0676A9A99 + 3) & M64))
    return sm64(h ^ (which + 4))


def bounded(r, rng):
    return (r * rng) >> 64


def draw_pos(seed, stream, S, m):
    """Rows of the edge list, 0-based (which = 0, attempt 0)."""
    return np.array([bounded(ctr_rand(seed, stream, k, 0, 0), m) for k in range(S)], dtype=np.int64)


def candidate(seed, stream, k, a, n, directed):
    i = bounded(ctr_rand(seed, stream, k, a, 1), n)
    j = bounded(ctr_rand(seed, stream, k, a, 2), n - 1)
    j += j >= i
    if not directed and i > j:
        i, j = j, i
    return i, j


def draw_neg(seed, stream, S, n, is_edge, directed, give_up=100000):
    """Per sample the first attempt whose pair is not an edge: (neg_i, neg_j, attempt), 0-based.  is_edge(i, j) takes the pair as
    the sampler keys it: i < j when undirected."""
    ni, nj, att = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    for k in range(S):
        for a in range(give_up):
            i, j = candidate(seed, stream, k, a, n, directed)
            if not is_edge(i, j):
                break
        else:
            raise AssertionError(f"sample {k}: no non-edge in {give_up} attempts")
        ni[k], nj[k], att[k] = i, j, a
    return ni, nj, att


def _mix(x):  # the hash the sampler places a candidate's key by
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def round_tables(seed, stream, n, directed, att):
    """What the open-addressing table of candidate keys holds in every round of the rejection, from the attempt numbers of a
    finished draw: round r holds the candidates of attempt r of the samples with att >= r, in a table of max(1024, the power of
    two >= 4 x their count) slots.  Linear probing fills the same SET of slots in any insertion order.  Per round a dict: cnt,
    size, distinct keys, duplicates (cnt - distinct), longest (run of occupied slots, cyclic), displaced (keys not in their home
    slot), wrapped (keys whose probing went past the end of the table to its start)."""
    out = []
    for r in range(int(att.max()) + 1):
        ks = np.flatnonzero(att >= r)
        keys = set()
        for k in ks:
            i, j = candidate(seed, stream, int(k), r, n, directed)
            keys.add((i << 32) | j)
        size = 1024
        while size < 4 * len(ks):
            size <<= 1
        occ = np.zeros(size, bool)
        displaced = wrapped = 0
        for key in sorted(keys):
            s = _mix(key) & (size - 1)
            home = s
            while occ[s]:
                s = (s + 1) & (size - 1)
            occ[s] = True
            displaced += s != home
            wrapped += s < home
        longest = run = 0
        for s in range(2 * size):
            run = run + 1 if occ[s & (size - 1)] else 0
            longest = max(longest, min(run, size))
        out.append(dict(cnt=len(ks), size=size, distinct=len(keys), duplicates=len(ks) - len(keys), longest=longest,
                        displaced=displaced, wrapped=wrapped))
    return out


# ---- the graphs of the draw tests: n = 48, edges by a fixed predicate on 0-based ids -------------------------------------------
DRAW_N, DRAW_SEED = 48, 11


def edge_u(i, j):  # undirected, about 75 % of the pairs
    return (i + j) % 4 != 0


def edge_d(i, j):  # directed and asymmetric, about 75 %
    return (i + 2 * j) % 4 != 0


def edge_dense(i, j):  # undirected, 87.5 %: a sample of seed 11 needs more attempts than the sampler's 64 rounds
    return (i + j) % 8 != 0


def edge_rows(pred, directed, n=DRAW_N):
    """The edge list of a predicate, 0-based (m, 2).  Undirected: one row per pair, every second one stored as (max, min)."""
    rows = [(i, j) for i in range(n) for j in (range(n) if directed else range(i + 1, n)) if i != j and pred(i, j)]
    rows = np.array(rows, np.int64)
    if not directed:
        flip = (rows[:, 0] + rows[:, 1]) % 2 == 1
        rows[flip] = rows[flip][:, ::-1]
    return rows


# ---- prepared pairs ----------------------------------------------------------------------------------------------------------
def prepare(src, dst, w, pos, pos2, ni, nj, directed):
    """The pairs the tallies read: the edge of every positive draw -- of pos2, the overwriting draw of :510, where there is one --
    with the weight of the FIRST draw, and the non-edges; (min, max) when undirected (:133).  w = None: a unit list."""
    rp = pos if pos2 is None else pos2
    a, b, u, v = src[rp], dst[rp], np.asarray(ni), np.asarray(nj)
    if not directed:
        a, b = np.minimum(a, b), np.maximum(a, b)
        u, v = np.minimum(u, v), np.maximum(u, v)
    wts = np.ones(len(pos)) if w is None else np.asarray(w, np.float64)[pos]
    return a, b, u, v, wts


# ---- dist() ------------------------------------------------------------------------------------------------------------------
def dist(X, i, j, hi):
    """dist(i, j) / hi of src/auxilary.jl:14-20 for vectors of pairs: fp64 differences and products, added in ascending k with
    one rounding per operation; 0 for i == j."""
    X = np.asarray(X, np.float64)
    i, j = np.asarray(i), np.asarray(j)
    df = X[i] - X[j]
    sq = df * df
    s = np.zeros(len(i))
    for k in range(X.shape[1]):
        s = s + sq[:, k]
    s = np.sqrt(s)
    s[i == j] = 0.0
    return s / hi


# ---- the tallies -------------------------------------------------------------------------------------------------------------
def values_landmark(Ta, Tb, v2l, vw, lw, i, j, d, alpha):
    """(T[l_i] vw_i / lw[l_i]) (T[l_j] vw_j / lw[l_j]) (1 - d)^alpha in long double (:187-189)."""
    Ta, Tb, vw, lw = (np.asarray(a, LD) for a in (Ta, Tb, vw, lw))
    li, lj = v2l[i], v2l[j]
    return (Ta[li] * vw[i] / lw[li]) * (Tb[lj] * vw[j] / lw[lj]) * (LD(1) - np.asarray(d, LD)) ** LD(alpha)


def values_exact(GD, Ta, Tb, i, j):
    """T_i T_j GD_ij in long double (:174, :205)."""
    return np.asarray(Ta, LD)[i] * np.asarray(Tb, LD)[j] * np.asarray(GD, LD)[i, j]


def gaps(pos, neg):
    """|pos - neg| / max(pos, neg) per sample (0 where both are 0)."""
    hi = np.maximum(pos, neg)
    return np.where(hi > 0, np.abs(pos - neg) / np.where(hi > 0, hi, 1), 0).astype(np.float64)


def slot_of(S, wide=None):
    """The slot of the 64 block tallies that sample k is added to.  Narrow grid (S < 65536): 64 blocks of 256 threads, sample
    k in block (k // 256) % 64.  Wide grid: block (k // 256) % 1024, folded into slot block // 16."""
    k = np.arange(S)
    wide = S >= WIDE_MIN if wide is None else wide
    return ((k // 256) % (BLOCKS * WIDE)) // WIDE if wide else (k // 256) % BLOCKS


def tally(pos, neg, wts, wide=None):
    """num[64], den[64] (long double), the samples per slot, and the totals {num, den} = the slots added up."""
    S = len(wts)
    w = np.asarray(wts, LD)
    slot = slot_of(S, wide)
    num, den = np.zeros(BLOCKS, LD), np.zeros(BLOCKS, LD)
    np.add.at(num, slot, np.where(pos > neg, w, LD(0)))
    np.add.at(den, slot, w)
    return num, den, np.bincount(slot, minlength=BLOCKS), (num.sum(), den.sum())


# ---- the inputs of the tally tests -------------------------------------------------------------------------------------------
def sample_weights(S):
    """Weights k / 4 that vary with the sample, so that no two slots hold the same sums."""
    k = np.arange(S)
    b = k // 256
    return ((k % 61) + (b * b + 3 * b) % 97 + 1) / 4.0


def random_pairs(rng, S, n, ordered):
    i = rng.integers(0, n, S)
    j = (i + rng.integers(1, n, S)) % n
    if not ordered:
        i, j = np.minimum(i, j), np.maximum(i, j)
    return i.astype(np.int32), j.astype(np.int32)


def interleaved_old2new(N, C):
    """Landmarks with community l % C, relabelled by community (members ascending): (comm, old2new)."""
    comm = np.arange(N) % C
    order = np.argsort(comm, kind="stable")
    old2new = np.empty(N, np.int32)
    old2new[order] = np.arange(N, dtype=np.int32)
    return comm, old2new


def exact_landmark_case(S, n=300, N=40, seed=1, directed=False):
    """Tier 1, landmark mode: every product, quotient and sum is exact in fp64 in any order at alpha = 1.  Sample k with
    k % 16 == 0 has the same pair and distance as pos and neg; the small value sets make many more ties by different factors."""
    rng = np.random.default_rng(seed)
    c = dict(N=N, alpha=1.0)
    c["v2l"] = np.concatenate((np.arange(N), rng.integers(0, N, n - N))).astype(np.int32)
    c["vw"] = rng.choice([0.5, 1.0, 2.0, 4.0], n)
    c["lweight"] = rng.choice([1.0, 2.0, 4.0], N)
    c["Ta"] = rng.choice([1.0, 1.5, 2.0, 3.0], N)
    c["Tb"] = rng.choice([1.0, 1.5, 2.0, 3.0], N) if directed else c["Ta"]
    pi, pj = random_pairs(rng, S, n, directed)
    ni, nj = random_pairs(rng, S, n, directed)
    dpos, dneg = rng.choice([0.0, 0.25, 0.5, 0.75], S), rng.choice([0.0, 0.25, 0.5, 0.75], S)
    same = np.arange(S) % 16 == 0
    ni[same], nj[same], dneg[same] = pi[same], pj[same], dpos[same]
    c["pairs"] = (pi, pj, ni, nj, sample_weights(S))
    c["dists"] = (dpos, dneg)
    return c


def exact_matrix_case(S, N=130, seed=2, directed=False):
    """Tier 1, exact mode: GD in {0, 1/4, .., 1} (symmetric when undirected), T in a small dyadic set; ties as above."""
    rng = np.random.default_rng(seed)
    GD = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], (N, N))
    if not directed:
        GD = np.triu(GD) + np.triu(GD, 1).T
    c = dict(N=N, GD=GD)
    c["Ta"] = rng.choice([1.0, 1.5, 2.0, 3.0], N)
    c["Tb"] = rng.choice([1.0, 1.5, 2.0, 3.0], N) if directed else c["Ta"]
    pi, pj = random_pairs(rng, S, N, directed)
    ni, nj = random_pairs(rng, S, N, directed)
    same = np.arange(S) % 16 == 0
    ni[same], nj[same] = pi[same], pj[same]
    c["pairs"] = (pi, pj, ni, nj, sample_weights(S))
    return c


def random_landmark_case(S, n=300, N=40, d=8, seed=3, directed=False):
    """Tier 2: continuous T, vw, lw, weights and an embedding for the distance stage; `hi` above every distance."""
    rng = np.random.default_rng(seed)
    c = dict(N=N, alpha=3.25)
    c["emb"] = rng.standard_normal((n, d))
    c["hi"] = float(2.0 * np.sqrt(d) * np.abs(c["emb"]).max() * 1.01)
    c["v2l"] = np.concatenate((np.arange(N), rng.integers(0, N, n - N))).astype(np.int32)
    c["vw"] = rng.random(n) + 0.5
    c["lweight"] = rng.random(N) * 5 + 1
    c["Ta"] = np.exp(rng.normal(size=N))
    c["Tb"] = np.exp(rng.normal(size=N)) if directed else c["Ta"]
    pi, pj = random_pairs(rng, S, n, directed)
    ni, nj = random_pairs(rng, S, n, directed)
    while True:  # no sample with one pair as pos and neg: that is an exact tie
        same = np.flatnonzero((pi == ni) & (pj == nj))
        if same.size == 0:
            break
        ni[same], nj[same] = random_pairs(rng, same.size, n, directed)
    c["pairs"] = (pi, pj, ni, nj, rng.random(S) + 0.1)
    return c


def sum_bound(terms, den):
    """The a-priori bound of a slot's fp64 sums against the exact ones: `terms` non-negative summands, each at most the slot's
    weight sum in all, added in any order with one rounding per addition -- at most terms x 2^-53 x the weight sum."""
    return np.asarray(terms * U * den, dtype=np.float64)
