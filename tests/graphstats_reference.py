"""A plain numpy restatement of the three rules of csrc/graphstats.hip, for the tests: min-id component labels by
union-find, breadth-first levels per source, and triangles by neighbour-set intersection.  Also the small graphs the CPU
and GPU test files share.  Nothing here touches the library under test."""
import networkx as nx
import numpy as np


def canonical_edges(n, edges):
    """(E, 2) int64 with u < v, unique, sorted: self-loops dropped, duplicates in either direction merged."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    assert len(e) == 0 or (e.min() >= 0 and e.max() < n)
    e = np.sort(e[e[:, 0] != e[:, 1]], axis=1)
    return np.unique(e, axis=0) if len(e) else e


def neighbours(n, edges):
    nb = [[] for _ in range(n)]
    for u, v in canonical_edges(n, edges).tolist():
        nb[u].append(v)
        nb[v].append(u)
    return nb


def component_labels(n, edges):
    """labels[v] = the smallest vertex id in v's component (union-find, the smaller root wins)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in canonical_edges(n, edges).tolist():
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(n)], dtype=np.int32).reshape(n)


def distances(n, edges, sources):
    """Per source: (reached, source included; sum of hop distances; greatest finite distance), by breadth-first levels."""
    nb = neighbours(n, edges)
    reached, dist_sum, ecc = [], [], []
    for s in np.asarray(sources, dtype=np.int64).tolist():
        seen = np.zeros(n, dtype=bool)
        seen[s] = True
        frontier, level, cnt, tot, far = [s], 0, 1, 0, 0
        while frontier:
            level += 1
            nxt = []
            for u in frontier:
                for w in nb[u]:
                    if not seen[w]:
                        seen[w] = True
                        nxt.append(w)
            if nxt:
                cnt += len(nxt)
                tot += level * len(nxt)
                far = level
            frontier = nxt
        reached.append(cnt)
        dist_sum.append(tot)
        ecc.append(far)
    return np.array(reached, dtype=np.int64), np.array(dist_sum, dtype=np.int64), np.array(ecc, dtype=np.int32)


def triangles(n, edges):
    """triangles[v] = triangles through v: over the edges (u, v), the common neighbours, each triangle seen from 3 edges."""
    sets = [set(r) for r in neighbours(n, edges)]
    t = np.zeros(n, dtype=np.int64)
    for u, v in canonical_edges(n, edges).tolist():
        for w in sets[u] & sets[v]:
            t[w] += 1
    return t


# ---- the graphs of tests/test_hip_graphstats.py, restated against networkx in tests/test_graphstats_cpu.py -----------
def permuted_path(n, seed=0):
    """A path whose vertex ids are a seeded random permutation."""
    p = np.random.default_rng(seed).permutation(n)
    return np.column_stack([p[:-1], p[1:]]).astype(np.int64)


def messy(n, edges, seed=0):
    """The same graph as an edge list that is shuffled, flipped, with duplicates and self-loops added."""
    rng = np.random.default_rng(seed)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if len(e):
        e = np.concatenate([e, e[rng.integers(0, len(e), size=len(e) // 2 + 1)][:, ::-1]])
    loops = rng.integers(0, n, size=5)
    e = np.concatenate([e, np.column_stack([loops, loops])])
    return e[rng.permutation(len(e))]


def edge_array(G):
    return np.array(list(G.edges()), dtype=np.int64).reshape(-1, 2)


CONNECTED = {
    "path50": lambda: nx.path_graph(50),
    "star300": lambda: nx.star_graph(299),
    "cycle101": lambda: nx.cycle_graph(101),
    "grid30": lambda: nx.convert_node_labels_to_integers(nx.grid_2d_graph(30, 30)),
    "k20": lambda: nx.complete_graph(20),
    "barbell": lambda: nx.barbell_graph(20, 1),
    "ws1000": lambda: nx.connected_watts_strogatz_graph(1000, 6, 0.1, seed=2),
    "n1": lambda: nx.empty_graph(1),
    "n2": lambda: nx.path_graph(2),
}

TRIANGLE_GRAPHS = {
    "k20": CONNECTED["k20"],
    "star300": CONNECTED["star300"],
    "wheel5001": lambda: nx.wheel_graph(5001),
    "caveman": lambda: nx.caveman_graph(10, 10),
    "ba1000": lambda: nx.barabasi_albert_graph(1000, 3, seed=1),
    "ws1000": CONNECTED["ws1000"],
}


def gnp2000():
    """35 components, the largest with 1965 vertices."""
    return nx.gnp_random_graph(2000, 0.002, seed=1)


def isolated_plus_edge():
    """300 isolated vertices and one edge between two more."""
    G = nx.empty_graph(302)
    G.add_edge(17, 301)
    return G
