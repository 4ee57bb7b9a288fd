"""Community structure on the GPU: Louvain communities, exact modularity and partition agreement.

louvain_communities, louvain_partitions and modularity carry networkx's names and argument forms.  The Louvain here is
the synchronous integer rule of include/graphem_hip.h "communities" (csrc/communities.hip: gh_cent_louvain), not
networkx's sequential sweep: partitions differ from networkx's as networkx's differ between seeds, at the same quality
(DESIGN.md section 18), and they are a pure function of (graph, seed, max_level) -- the same on every run and for every edge
order.  Modularity is the exact integer numerator N = M sum I - sum T^2 of gh_cent_modularity over M^2, one division of
two Python ints on the host.

Every function takes what CentralityGraph takes -- a networkx Graph, a scipy sparse adjacency (this package's graph type),
an (E, 2) edge array or a CentralityGraph.  Undirected, unweighted graphs only.  Self-loops are dropped and duplicate
edges merged.
"""
import math

import numpy as np

from .graphstats import _components_of, _unweighted, _with_graph

try:   # networkx is optional; its exception type is used when it is there
    from networkx.algorithms.community.quality import NotAPartition as _NotAPartition
except ImportError:   # pragma: no cover
    _NotAPartition = None

MAX_LEVELS = 32
MAX_ROUNDS = 1000


def _not_a_partition(G, communities):
    if _NotAPartition is not None:
        return _NotAPartition(G, communities)
    return ValueError(f"{communities} is not a valid partition of the graph")


def _plain(weight, resolution):
    _unweighted(weight)
    if resolution != 1:
        raise NotImplementedError("resolution must be 1")


def _labels_of(G, g, communities):
    """(n,) labels in [0, n) of `communities`: a label array over the vertices in vertex order, or an iterable of node
    sets, which must partition the nodes as networkx.community.is_partition asks."""
    if isinstance(communities, np.ndarray):
        labels = communities.ravel()
        if len(labels) != g.n or labels.dtype.kind not in "iub":
            raise _not_a_partition(G, communities)
        return np.unique(labels, return_inverse=True)[1].astype(np.int32).reshape(g.n)
    if not isinstance(communities, list):
        communities = list(communities)
    index = {v: i for i, v in enumerate(g.nodes)}
    labels = np.full(g.n, -1, dtype=np.int64)
    listed = 0
    for j, block in enumerate(communities):
        listed += len(block)
        for v in block:
            try:
                i = index.get(v)
            except TypeError:   # unhashable: no node
                i = None
            if i is not None:
                labels[i] = j
    if listed != g.n or (labels < 0).any():
        raise _not_a_partition(G, communities)
    return np.unique(labels, return_inverse=True)[1].astype(np.int32).reshape(g.n)   # empty blocks leave gaps


def modularity(G, communities, weight=None, resolution=1):
    """networkx.community.modularity on the GPU, for an unweighted graph at resolution 1: communities is an iterable of
    node sets, or an (n,) integer label array in vertex order.  Node sets that do not partition the nodes raise
    NotAPartition (ValueError without networkx); a graph without edges raises ZeroDivisionError, as networkx does."""
    _plain(weight, resolution)

    def run(g):
        sum_i, sum_t2, M = g.modularity_terms(_labels_of(G, g, communities))
        return (M * sum_i - sum_t2) / (M * M)
    return _with_graph(G, run)


def _levels(g, seed, max_level):
    if max_level is not None and (not isinstance(max_level, (int, np.integer)) or max_level <= 0):
        raise ValueError("max_level argument must be a positive integer or None")
    return g.louvain_levels(0 if seed is None else seed, MAX_LEVELS if max_level is None else int(max_level), MAX_ROUNDS)


def _node_sets(g, labels):
    nodes = g.nodes
    return [{nodes[i] for i in block} for block in _components_of(labels)]


def louvain_partitions(G, weight=None, resolution=1, threshold=None, seed=0, max_level=None):
    """The partition after every Louvain level, coarser and of larger modularity level by level, as a list of lists of
    node sets, each ordered by smallest member.  A graph whose first level merges nothing gives the singletons alone.
    threshold is ignored: a round is kept when it raises the exact integer numerator, and a level that merges nothing
    ends the run.  seed: an integer (None: 0)."""
    _plain(weight, resolution)
    del threshold
    return _with_graph(G, lambda g: [_node_sets(g, row) for row in _levels(g, seed, max_level)[0]])


def louvain_communities(G, weight=None, resolution=1, threshold=None, seed=0, max_level=None):
    """networkx.community.louvain_communities on the GPU: the last of louvain_partitions, a list of node sets ordered by
    smallest member ([] for the null graph)."""
    _plain(weight, resolution)
    del threshold

    def run(g):
        labels = _levels(g, seed, max_level)[0]
        return _node_sets(g, labels[-1]) if len(labels) else []
    return _with_graph(G, run)


def community_labels(G, seed=0, level=-1):
    """(n,) int32: the smallest vertex id in every vertex's Louvain community after `level` (-1: the last), in vertex
    order -- for node_colors and for comparison with planted labels such as generate_sbm(labels=True)."""
    def run(g):
        labels = _levels(g, seed, None)[0]
        return labels[level].copy() if len(labels) else np.zeros(0, dtype=np.int32)
    return _with_graph(G, run)


def _pairs_within(counts):
    """sum of C(c, 2) over the int64 counts, a Python int."""
    return int((counts * (counts - 1) // 2).sum())


def adjusted_rand_index(a, b):
    """The adjusted Rand index of two labellings of the same items (any integer or hashable labels), on the host.  The
    contingency table comes from the sorted label pairs; with P = C(n, 2), S = sum C(n_ij, 2), A and B the same sums over
    the row and column totals, the index is 2 (S P - A B) / ((A + B) P - 2 A B): exact integers and one division.  Two
    identical trivial partitions (all singletons, or one block; also n < 2) make the denominator 0 and give 1.0."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    if len(a) != len(b):
        raise ValueError("the two labellings must have the same length")
    n = len(a)
    ia = np.unique(a, return_inverse=True)[1].astype(np.int64).reshape(n)
    ib = np.unique(b, return_inverse=True)[1].astype(np.int64).reshape(n)
    pair = np.sort(ia * (int(ib.max()) + 1 if n else 1) + ib)
    cells = np.diff(np.flatnonzero(np.r_[True, pair[1:] != pair[:-1], True])) if n else np.zeros(0, dtype=np.int64)
    S, A, B = _pairs_within(cells.astype(np.int64)), _pairs_within(np.bincount(ia)), _pairs_within(np.bincount(ib))
    P = n * (n - 1) // 2
    den = (A + B) * P - 2 * A * B
    return 1.0 if den == 0 else 2 * (S * P - A * B) / den


def normalized_mutual_info(a, b):
    """The normalised mutual information of two labellings of the same items (any integer or hashable labels), on the host,
    in natural logarithms with the arithmetic mean of the entropies: NMI = MI / ((H(a) + H(b)) / 2).  The integer contingency
    cells n_ij come from the sorted label pairs, as for adjusted_rand_index; with the row and column totals a_i and b_j,
    MI = fsum over the cells of (n_ij / n) log((n n_ij) / (a_i b_j)) and H(a) = fsum of (a_i / n) log(n / a_i), the products
    in integers and every sum a math.fsum.  Identical labellings give the same terms on both sides, so exactly 1.0; two
    trivial labellings (both entropies 0; also n = 0) give 1.0; one trivial labelling gives 0.0."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    if len(a) != len(b):
        raise ValueError("the two labellings must have the same length")
    n = len(a)
    if n == 0:
        return 1.0
    ia = np.unique(a, return_inverse=True)[1].astype(np.int64).reshape(n)
    ib = np.unique(b, return_inverse=True)[1].astype(np.int64).reshape(n)
    kb = int(ib.max()) + 1
    pair = np.sort(ia * kb + ib)
    first = np.flatnonzero(np.r_[True, pair[1:] != pair[:-1], True])
    cells, key = np.diff(first), pair[first[:-1]]
    ra, rb = np.bincount(ia), np.bincount(ib)

    def entropy(t):
        return math.fsum((t / n * np.log(n / t)).tolist())
    ha, hb = entropy(ra), entropy(rb)
    if ha == 0.0 and hb == 0.0:
        return 1.0
    mi = math.fsum((cells / n * np.log((n * cells) / (ra[key // kb] * rb[key % kb]))).tolist())
    return mi / ((ha + hb) / 2)
