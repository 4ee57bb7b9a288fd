"""A plain numpy / Python restatement of the two rules of csrc/cores.hip (include/graphem_hip.h "cores and trusses"), for
the tests: the synchronous vertex peel (core number, onion layer) and the synchronous edge peel (truss number).  Also the
graphs the CPU and GPU test files share, with the values pinned for them.  Nothing here touches the library under test."""
import functools

import networkx as nx
import numpy as np

import graphstats_reference as gsr
from graphstats_reference import canonical_edges, edge_array, messy, permuted_path   # noqa: F401  (shared with the tests)


def peel(n, edges):
    """(core (n,) int32, layer (n,) int32, rounds) of the vertex peel."""
    e = canonical_edges(n, edges)
    u, v = (e[:, 0], e[:, 1]) if len(e) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    deg = np.bincount(e.ravel(), minlength=n).astype(np.int64)
    alive = np.ones(n, dtype=bool)
    core, layer = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    k = r = 0
    while alive.any():
        r += 1
        k = max(k, int(deg[alive].min()))
        S = alive & (deg <= k)
        core[S], layer[S] = k, r
        alive &= ~S
        deg -= np.bincount(v[S[u] & alive[v]], minlength=n) + np.bincount(u[S[v] & alive[u]], minlength=n)
    return core, layer, r


def truss(n, edges):
    """(edges (E, 2) int64 canonical, truss (E,) int32, rounds) of the edge peel.  After every round the decremented
    supports are checked against a fresh count over the alive edges."""
    e = canonical_edges(n, edges)
    m = len(e)
    pairs = [tuple(p) for p in e.tolist()]
    index = {p: i for i, p in enumerate(pairs)}
    nb = [set() for _ in range(n)]   # alive neighbours
    for a, b in pairs:
        nb[a].add(b)
        nb[b].add(a)

    def eid(a, b):
        return index[(a, b) if a < b else (b, a)]

    sup = np.array([len(nb[a] & nb[b]) for a, b in pairs], dtype=np.int64).reshape(m)
    alive = np.ones(m, dtype=bool)
    out = np.zeros(m, dtype=np.int32)
    j = r = 0
    while alive.any():
        r += 1
        j = max(j, int(sup[alive].min()))
        in_s = alive & (sup <= j)
        S = np.flatnonzero(in_s).tolist()
        out[S] = j + 2
        for i in S:   # every triangle alive at the start of the round, at its smallest-id edge of S
            a, b = pairs[i]
            for w in nb[a] & nb[b]:
                e1, e2 = eid(a, w), eid(b, w)
                if (in_s[e1] and e1 < i) or (in_s[e2] and e2 < i):
                    continue
                if not in_s[e1]:
                    sup[e1] -= 1
                if not in_s[e2]:
                    sup[e2] -= 1
        for i in S:
            a, b = pairs[i]
            nb[a].discard(b)
            nb[b].discard(a)
        alive[S] = False
        for i in np.flatnonzero(alive).tolist():
            a, b = pairs[i]
            assert sup[i] == len(nb[a] & nb[b]), (r, i)
    return e, out, r


# ---- the graphs of tests/test_hip_cores.py, restated against networkx in tests/test_cores_cpu.py ---------------------
def _path5000():
    G = nx.empty_graph(5000)
    G.add_edges_from(permuted_path(5000).tolist())
    return G


def _plc_gnp_caveman():
    """The base that tests/tiled_graphs.py tiles to a million vertices: cores 0 .. 9 without 5 and 6, trusses 2 .. 9, 28
    components and 5467 triangles on 2360 vertices and 7952 edges."""
    return nx.disjoint_union_all([nx.powerlaw_cluster_graph(1000, 4, 0.3, seed=5), nx.gnp_random_graph(1000, 0.004, seed=1),
                                  nx.relaxed_caveman_graph(30, 12, 0.15, seed=3)])


GRAPHS = {
    "plc_gnp_caveman": _plc_gnp_caveman,
    "path5000": _path5000,
    "lollipop": lambda: nx.lollipop_graph(40, 700),
    "wheel5001": gsr.TRIANGLE_GRAPHS["wheel5001"],
    "gnp2000": gsr.gnp2000,
    "gnp600": lambda: nx.gnp_random_graph(600, 0.1, seed=4),
    "gnp300": lambda: nx.gnp_random_graph(300, 0.25, seed=7),
    "relaxed_caveman": lambda: nx.relaxed_caveman_graph(30, 12, 0.15, seed=3),
    "plc3000": lambda: nx.powerlaw_cluster_graph(3000, 4, 0.3, seed=5),
    "barbell": gsr.CONNECTED["barbell"],
    "k20": gsr.CONNECTED["k20"],
    "caveman": gsr.TRIANGLE_GRAPHS["caveman"],
    "star300": gsr.CONNECTED["star300"],
    "cycle101": gsr.CONNECTED["cycle101"],
    "grid30": gsr.CONNECTED["grid30"],
    "ws1000": gsr.CONNECTED["ws1000"],
    "ba1000": gsr.TRIANGLE_GRAPHS["ba1000"],
    "isolated": gsr.isolated_plus_edge,
    "n1": gsr.CONNECTED["n1"],
    "n2": gsr.CONNECTED["n2"],
    "null": nx.Graph,
}

VERTEX_GRAPHS = ["path5000", "lollipop", "wheel5001", "gnp2000", "gnp600", "relaxed_caveman", "barbell", "k20", "caveman",
                 "star300", "cycle101", "grid30", "ws1000", "ba1000", "isolated", "n1", "n2", "null"]
EDGE_GRAPHS = ["k20", "barbell", "relaxed_caveman", "gnp300", "gnp600", "wheel5001", "plc3000", "grid30", "path5000",
               "isolated", "n1"]

# name: (n, E, degeneracy, onion layers)
VERTEX_PINS = {
    "path5000": (5000, 4999, 1, 2500),
    "lollipop": (740, 1480, 39, 701),
    "wheel5001": (5001, 10000, 3, 2),
    "gnp2000": (2000, 3989, 3, 15),
    "gnp600": (600, 17827, 46, 26),
    "relaxed_caveman": (360, 1980, 9, 49),
}
# name: (E, max truss, rounds)
EDGE_PINS = {
    "k20": (190, 20, 1),
    "barbell": (382, 20, 2),
    "relaxed_caveman": (1980, 9, 25),
    "gnp300": (11232, 13, 58),
    "gnp600": (17827, 5, 23),
    "wheel5001": (10000, 3, 2),
    "plc3000": (11981, 5, 11),
    "grid30": (1740, 2, 1),
    "path5000": (4999, 2, 1),
    "isolated": (1, 2, 1),
    "n1": (0, 0, 0),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    """(networkx graph, n, (E, 2) int64 edges as networkx lists them)."""
    G = GRAPHS[name]()
    return G, G.number_of_nodes(), edge_array(G)


@functools.lru_cache(maxsize=None)
def peel_of(name):
    """peel() of a named graph, computed once; callers leave the arrays unchanged."""
    _, n, e = graph(name)
    return peel(n, e)


@functools.lru_cache(maxsize=None)
def truss_of(name):
    """truss() of a named graph, computed once; callers leave the arrays unchanged."""
    _, n, e = graph(name)
    return truss(n, e)
