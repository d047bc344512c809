"""Small graphs with known communities for the Louvain tests -- TEST INFRASTRUCTURE, numpy only.
Every generator returns (edges0 (m, 2) int64 0-based, n)."""
import numpy as np


def _e(pairs):
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def path(n):
    return _e([(i, i + 1) for i in range(n - 1)]), n


def cycle(n):
    return _e([(i, (i + 1) % n) for i in range(n)]), n


def star(leaves):
    return _e([(0, i) for i in range(1, leaves + 1)]), leaves + 1


def clique(first, size):
    return [(first + i, first + j) for i in range(size) for j in range(i + 1, size)]


def clique_chain(cliques, size, ring=False):
    """`cliques` K_size in a row, the last vertex of each joined to the first vertex of the next (and round again: ring)."""
    pairs = []
    for c in range(cliques):
        pairs += clique(c * size, size)
    for c in range(cliques if ring else cliques - 1):
        pairs.append((c * size + size - 1, ((c + 1) % cliques) * size))
    return _e(pairs), cliques * size


def clique_labels(cliques, size):
    return np.repeat(np.arange(cliques), size)


def barbell(a, inner):
    """Two K_a joined by a path with `inner` vertices between them (0: one bridge edge)."""
    chain = [a - 1] + [2 * a + i for i in range(inner)] + [a]
    return _e(clique(0, a) + clique(a, a) + list(zip(chain[:-1], chain[1:]))), 2 * a + inner


def random_multigraph(n, seed):
    """About 3n edges on n vertices: repeated edges, self loops, and (from n = 8) vertices that no edge touches."""
    rng = np.random.default_rng(seed)
    live = np.arange(n) if n < 8 else rng.permutation(n)[: n - max(1, n // 16)]
    m = 3 * n
    e = live[rng.integers(0, len(live), size=(m, 2))]
    loops = rng.random(m) < 0.08
    e[loops, 1] = e[loops, 0]
    dup = rng.integers(0, m, size=m // 8)  # repeat some edges, the other way round
    e[dup] = e[rng.integers(0, m, size=m // 8)][:, ::-1]
    return e.astype(np.int64), n


def star_of_cliques(groups=1000, size=5):
    """A hub joined to groups * size leaves, the leaves forming `groups` K_size: one long adjacency segment among short."""
    leaves = groups * size
    pairs = [(0, i) for i in range(1, leaves + 1)]
    for g in range(groups):
        pairs += clique(1 + g * size, size)
    return _e(pairs), leaves + 1


def weighted_clique_ring(cliques, size, intra=1.3, bridge=0.7):
    """A ring of cliques with real weights, one repeated edge, three self loops, a vertex with only a self loop and an
    isolated vertex (the last two ids).  Returns (edges0, w, n, labels): the communities a correct pass must find."""
    e, n0 = clique_chain(cliques, size, ring=True)
    n_intra = cliques * size * (size - 1) // 2
    w = np.concatenate([np.full(n_intra, intra), np.full(len(e) - n_intra, bridge)])
    extra = [(1, 0), (2, 2), (size, size), (n0 - 1, n0 - 1), (n0, n0)]  # (1, 0) repeats the first clique's first edge
    e = np.concatenate([e, _e(extra)])
    w = np.concatenate([w, [intra, 0.5, 0.9, 0.4, 1.1]])
    labels = np.concatenate([clique_labels(cliques, size), [cliques, cliques + 1]])
    return e, w, n0 + 2, labels
