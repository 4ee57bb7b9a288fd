"""A plain numpy restatement of the Louvain rule of include/graphem_hip.h ("communities"): level graphs with exact integer
weights, rounds of best moves computed from the labels at the start of the round, the priority words that pick pairwise
non-adjacent movers, the exact numerator N = M sum I - sum T^2 that accepts or discards a round, and aggregation.  Also
the partition-agreement index by brute force and the graphs the CPU and GPU test files share.  Nothing here touches the
library under test."""
import numpy as np

import graphem_rapids_amd as gr
from graphstats_reference import canonical_edges, messy   # noqa: F401  (shared with the test files)

GOLDEN = 0x9E3779B97F4A7C15
_MASK = (1 << 64) - 1


def mix(z):
    """The header's mix() on a uint64 array (wrapping)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def priorities(seed, level, r, n):
    base = mix(np.array([(int(seed) + int(level) * GOLDEN) & _MASK], dtype=np.uint64))[0]
    ids = (np.uint64(r) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return mix(base ^ ids)


def _sum_by_key(key, values):
    """(unique keys ascending, exact int64 sums of values per key)."""
    if len(key) == 0:
        return key, values
    order = np.argsort(key, kind="stable")
    key, values = key[order], values[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    return key[starts], np.add.reduceat(values, starts)


def _scatter_sum(index, values, size):
    out = np.zeros(size, dtype=np.int64)
    np.add.at(out, index, values)
    return out


def numerator_terms(n, src, dst, w, s, k, c):
    """(sum I, sum T^2) of labelling c on a level graph, as Python ints."""
    same = c[src] == c[dst]
    T = _scatter_sum(c, k, n)
    return int(s.sum()) + int(w[same].sum()), sum(int(t) * int(t) for t in T[T > 0])


def one_level(n, src, dst, w, s, k, M, seed, level, max_rounds):
    """Rounds of one level from singletons: (labels, N, rounds, accepted numerators)."""
    c = np.arange(n, dtype=np.int64)
    T = k.copy()
    sI, sT2 = numerator_terms(n, src, dst, w, s, k, c)
    N = M * sI - sT2
    fails, rounds, trail = 0, 0, []
    for r in range(max_rounds):
        rounds += 1
        key, W = _sum_by_key(src * n + c[dst], w)
        u, d = key // max(n, 1), key % max(n, 1)
        own = d == c[u]
        W_own = np.zeros(n, dtype=np.int64)
        W_own[u[own]] = W[own]
        stay = M * W_own - k * (T[c] - k)
        u, d, W = u[~own], d[~own], W[~own]
        val = M * W - k[u] * T[d]
        order = np.lexsort((d, -val, u))
        u, d, val = u[order], d[order], val[order]
        first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]]) if len(u) else np.zeros(0, dtype=np.int64)
        target = c.copy()
        bu, bd, bv = u[first], d[first], val[first]
        better = bv > stay[bu]
        target[bu[better]] = bd[better]
        want = target != c
        if not want.any():
            break
        prio = priorities(seed, level, r, n)
        both = want[src] & want[dst]
        a, b = src[both], dst[both]
        beaten = (prio[b] > prio[a]) | ((prio[b] == prio[a]) & (b > a))
        mover = want.copy()
        mover[a[beaten]] = False
        c2 = np.where(mover, target, c)
        sI2, sT22 = numerator_terms(n, src, dst, w, s, k, c2)
        N2 = M * sI2 - sT22
        if N2 > N:
            c, N, fails = c2, N2, 0
            T = _scatter_sum(c, k, n)
            trail.append(N)
        else:
            fails += 1
            if fails == 2:
                break
    return c, N, rounds, trail


def aggregate(n, src, dst, w, s, k, c):
    """The coarse level graph of labelling c: (n', src', dst', w', s', k', comp) with comp[u] = u's coarse vertex."""
    ids = np.unique(c)
    comp = np.searchsorted(ids, c)
    m = len(ids)
    key, W = _sum_by_key(comp[src] * m + comp[dst], w)
    a, b = key // max(m, 1), key % max(m, 1)
    diag = a == b
    s2 = _scatter_sum(comp, s, m)
    s2[a[diag]] += W[diag]
    return m, a[~diag], b[~diag], W[~diag], s2, _scatter_sum(comp, k, m), comp


def min_member_labels(comp):
    """label[v] = the smallest v' with comp[v'] == comp[v]."""
    n = len(comp)
    low = np.full(int(comp.max()) + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(low, comp, np.arange(n))
    return low[comp].astype(np.int32)


def louvain(n, edges, seed=0, max_levels=32, max_rounds=1000, trails=None):
    """The rule end to end: (labels (L, n) int32, numerators [L], n_communities [L], rounds [L], M).  L >= 1: when level 0
    merges nothing the one labelling is the singletons.  trails (a list) receives every level's accepted numerators."""
    e = canonical_edges(n, edges)
    src = np.concatenate([e[:, 0], e[:, 1]])
    dst = np.concatenate([e[:, 1], e[:, 0]])
    M = len(src)
    w = np.ones(M, dtype=np.int64)
    s = np.zeros(n, dtype=np.int64)
    k = _scatter_sum(src, w, n)
    of_vertex = np.arange(n, dtype=np.int64)
    nl = n
    labels, numerators, counts, rounds = [], [], [], []
    for level in range(max_levels):
        c, N, rr, trail = one_level(nl, src, dst, w, s, k, M, seed, level, max_rounds)
        m, src2, dst2, w2, s2, k2, comp = aggregate(nl, src, dst, w, s, k, c)
        if m == nl:
            if level == 0:
                labels.append(np.arange(n, dtype=np.int32))
                numerators.append(N)
                counts.append(n)
                rounds.append(rr)
            break
        if trails is not None:
            trails.append(trail)
        of_vertex = comp[of_vertex]
        labels.append(min_member_labels(of_vertex))
        numerators.append(N)
        counts.append(m)
        rounds.append(rr)
        nl, src, dst, w, s, k = m, src2, dst2, w2, s2, k2
    return np.array(labels, dtype=np.int32).reshape(len(labels), n), numerators, counts, rounds, M


def modularity_terms(n, edges, labels):
    """(sum I, sum T^2, M) of a labelling of the original vertices, as Python ints."""
    e = canonical_edges(n, edges)
    labels = np.asarray(labels, dtype=np.int64)
    deg = np.bincount(e.ravel(), minlength=n).astype(np.int64)
    inside = 2 * int((labels[e[:, 0]] == labels[e[:, 1]]).sum())
    T = _scatter_sum(labels, deg, n) if n else np.zeros(0, dtype=np.int64)
    return inside, sum(int(t) * int(t) for t in T[T > 0]), 2 * len(e)


def q_of(terms):
    sI, sT2, M = terms
    return (M * sI - sT2) / (M * M)


def pair_count_ari(a, b):
    """The adjusted Rand index by counting vertex pairs one by one (n <= 60 or so)."""
    from fractions import Fraction
    n = len(a)
    both = in_a = in_b = 0
    for i in range(n):
        for j in range(i + 1, n):
            sa, sb = a[i] == a[j], b[i] == b[j]
            both += sa and sb
            in_a += sa
            in_b += sb
    pairs = n * (n - 1) // 2
    num = Fraction(both) - Fraction(in_a * in_b, pairs) if pairs else Fraction(0)
    den = Fraction(in_a + in_b, 2) - Fraction(in_a * in_b, pairs) if pairs else Fraction(0)
    return 1.0 if den == 0 else float(num / den)


# ---- the graphs of tests/test_communities_cpu.py and tests/test_hip_communities.py -----------------------------------
def _block_matrix(blocks, p_in, p_out):
    P = np.full((blocks, blocks), p_out)
    np.fill_diagonal(P, p_in)
    return P


def _block_labels(sizes):
    starts = np.cumsum([0] + list(sizes[:-1]))
    return np.repeat(starts, sizes).astype(np.int32)


def planted():
    """name -> (n, edges, planted min-id labels)."""
    a, b = [200] * 8, [40, 60, 80, 100, 120, 200]
    return {
        "sbm8": (1600, gr.sbm_edges(a, _block_matrix(8, 0.1, 0.005), 1), _block_labels(a)),
        "sbm6": (600, gr.sbm_edges(b, _block_matrix(6, 0.3, 0.01), 7), _block_labels(b)),
        "caveman": (100, gr.caveman_edges(10, 10), _block_labels([10] * 10)),
        "relaxed": (240, gr.relaxed_caveman_edges(20, 12, 0.1, seed=3), _block_labels([12] * 20)),
    }


def quality_graphs():
    """name -> (n, edges): the graphs whose final modularity is held against networkx's Louvain."""
    return {
        "gnp3000": (3000, gr.erdos_renyi_edges(3000, 0.002, seed=5)),
        "ba3000": (3000, gr.barabasi_albert_edges(3000, 3, seed=2)),
        "ws2000": (2000, gr.watts_strogatz_edges(2000, 6, 0.1, seed=4)),
        "road40": (1600, gr.road_network_edges(40, 40)),
        "tree2_9": (2 ** 10 - 1, gr.balanced_tree_edges(2, 9)),
        "regular2000": (2000, gr.random_regular_edges(2000, 4, seed=1)),
    }


def _complete(ids):
    ids = np.asarray(ids)
    i, j = np.triu_indices(len(ids), 1)
    return np.column_stack([ids[i], ids[j]])


def edge_cases():
    """name -> (n, edges)."""
    empty = np.zeros((0, 2), dtype=np.int64)
    two_triangles = np.array([[0, 1], [1, 2], [0, 2], [3, 4], [4, 5], [3, 5], [2, 3]])
    return {
        "n1": (1, empty),
        "n2": (2, np.array([[0, 1]])),
        "no_edges": (7, empty),
        "triangle_isolated": (5, np.array([[1, 2], [2, 4], [1, 4]])),
        "two_triangles": (6, two_triangles),
        "k20": (20, _complete(np.arange(20))),
        "k8_12": (20, np.array([[a, 8 + b] for a in range(8) for b in range(12)])),
        "star200": (201, np.column_stack([np.zeros(200, dtype=np.int64), np.arange(1, 201)])),
    }


LADDER_DEGREES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257]


def degree_ladder():
    """(n, edges): one star per degree of LADDER_DEGREES, a hub with 5000 leaves, and a hub whose 5000 leaves sit in
    cliques of 3 (1666 triangles and one pair), so that its row sees about 1700 distinct communities once they merge."""
    parts, n = [], 0
    for d in LADDER_DEGREES + [5000]:
        parts.append(np.column_stack([np.full(d, n, dtype=np.int64), n + 1 + np.arange(d)]))
        n += d + 1
    hub, leaves = n, n + 1 + np.arange(5000)
    parts.append(np.column_stack([np.full(5000, hub, dtype=np.int64), leaves]))
    tri = leaves[:4998].reshape(-1, 3)
    parts += [tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [0, 2]], leaves[4998:].reshape(1, 2)]
    return n + 5001, np.concatenate(parts)


def ring(n):
    v = np.arange(n, dtype=np.int64)
    return n, np.column_stack([v, (v + 1) % n])
