"""A plain Python / numpy restatement of the rule of csrc/links.hip (include/graphem_hip.h "link scores"), for the tests:
neighbour sets and dicts, the fixed-point weights taken from the library's own gh_link_weight (a host function, no device),
candidates by set algebra and the total order by sorting exact fractions.  Also the graphs the CPU and GPU test files
share.  Nothing else here touches the library under test."""
import functools
from fractions import Fraction

import networkx as nx
import numpy as np

from graphem_rapids_amd import _native

from graphstats_reference import canonical_edges, edge_array, messy   # noqa: F401  (shared with the tests)

KINDS = ["common_neighbors", "jaccard", "adamic_adar", "resource_allocation", "preferential_attachment"]
CN, JACCARD, AA, RA, PA = range(5)
SCALE = 1 << 32


@functools.lru_cache(maxsize=None)
def weight(kind, degree):
    return _native.link_weight(kind, degree)


def neighbour_sets(n, edges):
    nb = [set() for _ in range(n)]
    for u, v in canonical_edges(n, edges).tolist():
        nb[u].add(v)
        nb[v].add(u)
    return nb


def _sums(nb, u, v):
    """(cn, aa, ra, uni, pa) of one pair, Python ints."""
    common = nb[u] & nb[v]
    cn = len(common)
    aa = sum(weight(AA, len(nb[w])) for w in common)
    ra = sum(weight(RA, len(nb[w])) for w in common)
    return cn, aa, ra, len(nb[u]) + len(nb[v]) - cn, len(nb[u]) * len(nb[v])


def pair_scores(n, edges, pairs):
    """{'cn', 'aa', 'ra', 'uni', 'pa'}: (P,) int64 arrays of the vertex-id pairs."""
    nb = neighbour_sets(n, edges)
    rows = [_sums(nb, u, v) for u, v in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()]
    cols = np.array(rows, dtype=np.int64).reshape(-1, 5)
    return dict(zip(("cn", "aa", "ra", "uni", "pa"), cols.T.copy()))


def key_of(kind, sums):
    """(num, den) of the rational key of score kind `kind` from _sums' tuple."""
    cn, aa, ra, uni, pa = sums
    return {CN: (cn, 1), JACCARD: (cn, uni), AA: (aa, 1), RA: (ra, 1), PA: (pa, 1)}[kind]


def ranked_candidates(n, edges, kind):
    """Per vertex u the whole of C(u) as a list of (v, num, den), best first: key descending, then id ascending."""
    nb = neighbour_sets(n, edges)
    out = []
    for u in range(n):
        two_hop = set().union(*(nb[w] for w in nb[u])) - nb[u] - {u} if nb[u] else set()
        entries = [(v,) + key_of(kind, _sums(nb, u, v)) for v in two_hop]
        entries.sort(key=lambda e: (-Fraction(e[1], e[2]), e[0]))
        out.append(entries)
    return out


def candidates(ranked, k, rows):
    """(ids (R, k) int32, num (R, k) int64, den (R, k) int64) from ranked_candidates' lists; unused slots -1, 0, 1."""
    rows = list(rows)
    ids = np.full((len(rows), k), -1, dtype=np.int32)
    num = np.zeros((len(rows), k), dtype=np.int64)
    den = np.ones((len(rows), k), dtype=np.int64)
    for r, u in enumerate(rows):
        for j, (v, a, b) in enumerate(ranked[u][:k]):
            ids[r, j], num[r, j], den[r, j] = v, a, b
    return ids, num, den


# ---- the graphs ------------------------------------------------------------------------------------------------------
HUB, A63, B64, C65, LONE = 0, 301, 302, 303, 304


def _row_lengths():
    """Rows of length 300 (the hub 0 over the leaves 1 .. 300), 63, 64 and 65 (vertices 301, 302, 303 over the first 63, 64
    and 65 leaves), 4, 3, 2 and 1 (the leaves) and 0 (vertex 304)."""
    G = nx.empty_graph(305)
    G.add_edges_from((HUB, leaf) for leaf in range(1, 301))
    for v, length in ((A63, 63), (B64, 64), (C65, 65)):
        G.add_edges_from((v, leaf) for leaf in range(1, length + 1))
    return G


def _triangle_tail():
    """Triangle 0-1-2 with the tail 2-3-4: from 0, vertex 1 is adjacent AND two hops away (through 2)."""
    return nx.Graph([(0, 1), (1, 2), (2, 0), (2, 3), (3, 4)])


def _star_path():
    """A 40-leaf star at 0 whose leaf 40 starts a path of 10 more vertices."""
    G = nx.star_graph(40)
    nx.add_path(G, range(40, 51))
    return G


def _n65():
    return nx.gnp_random_graph(65, 0.15, seed=6)


def _isolated_source():
    G = nx.cycle_graph(6)
    G.add_node(6)
    return G


GRAPHS = {
    "rows": _row_lengths,
    "k5": lambda: nx.complete_graph(5),
    "triangle_tail": _triangle_tail,
    "c7": lambda: nx.cycle_graph(7),
    "k34": lambda: nx.complete_bipartite_graph(3, 4),
    "star300": lambda: nx.star_graph(300),
    "ba300": lambda: nx.barabasi_albert_graph(300, 4, seed=1),
    "caveman": lambda: nx.relaxed_caveman_graph(8, 9, 0.2, seed=2),
    "star_path": _star_path,
    "isolated_source": _isolated_source,
    "n65": _n65,
    "dense130": lambda: nx.gnp_random_graph(130, 0.5, seed=3),
}
# the graphs of the candidate tests; BIG ones are run over all their vertices at every k
CANDIDATE_GRAPHS = ["k5", "triangle_tail", "c7", "k34", "star300", "ba300", "caveman", "isolated_source", "n65", "rows"]
NETWORKX_GRAPHS = ["ba300", "caveman", "star_path", "k5", "triangle_tail", "c7", "k34", "isolated_source", "n65", "star300",
                   "rows", "dense130"]


@functools.lru_cache(maxsize=None)
def graph(name):
    """(networkx graph, n, (E, 2) int64 edges as networkx lists them)."""
    G = GRAPHS[name]()
    return G, G.number_of_nodes(), edge_array(G)


@functools.lru_cache(maxsize=None)
def ranked_of(name, kind):
    """ranked_candidates() of a named graph, computed once; callers leave the lists unchanged."""
    _, n, e = graph(name)
    return ranked_candidates(n, e, kind)


def all_pairs(n):
    """Every pair u <= v: the pairs with u = v included."""
    u, v = np.triu_indices(n)
    return np.column_stack([u, v]).astype(np.int64)


def row_length_pairs():
    """Pairs over the "rows" graph: every combination of the row lengths 0, 1, 2, 3, 4, 63, 64, 65 and 300 in both orders
    (u = v included), adjacent pairs, pairs with the isolated vertex, and repeats, shuffled."""
    pick = [LONE, 300, 65, 64, 1, 2, A63, B64, C65, HUB]
    pairs = [(a, b) for a in pick for b in pick]
    pairs += [(HUB, 7), (7, HUB), (A63, 63), (C65, 65), (5, 9), (9, 5), (200, 201), (LONE, LONE)]
    pairs += pairs[::3]
    pairs = np.array(pairs, dtype=np.int64)
    return pairs[np.random.default_rng(11).permutation(len(pairs))]
