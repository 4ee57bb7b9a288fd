"""Core and truss decomposition on the GPU: the k-shell structure of a graph under networkx's names.

core_number, onion_layers, k_core / k_shell / k_crust / k_corona and k_truss with networkx's results, plus degeneracy and
truss_number (the largest k whose k-truss holds an edge).  Two integer-exact synchronous peels in HIP over the centrality
handle's CSR do the work (csrc/cores.hip: gh_cent_cores gives core numbers and onion layers from one pass, gh_cent_truss
the truss number of every edge); include/graphem_hip.h "cores and trusses" states both rules.

Every function takes what CentralityGraph takes -- a networkx Graph, a scipy sparse adjacency (this package's graph type),
an (E, 2) edge array or a CentralityGraph -- and results are keyed by node.  The subgraph functions return this package's
graph type as largest_connected_component does: the induced symmetric CSR of ones, its vertices relabelled to 0 .. m-1 in
ascending original id, and with return_vertices=True also the original ids (nodes for a labelled networkx graph).
Undirected, unweighted graphs only.  A networkx Graph with self-loops raises NetworkXNotImplemented as networkx does;
arrays and matrices drop self-loops silently, like the rest of the package.
"""
import numpy as np

from .centrality import _nx
from .generators import edges_to_adjacency
from .graphstats import _induced_edges, _with_graph

_CORE_LOOPS = ("Input graph has self loops which is not permitted; "
               "Consider using G.remove_edges_from(nx.selfloop_edges(G)).")
_ONION_LOOPS = ("Input graph contains self loops which is not permitted; "
                "Consider using G.remove_edges_from(nx.selfloop_edges(G)).")


def _no_selfloops(G, msg):
    """networkx's refusal of a Graph with self-loops, on the host, before a handle exists."""
    if _nx is not None and isinstance(G, _nx.Graph) and _nx.number_of_selfloops(G) > 0:
        raise _nx.NetworkXNotImplemented(msg)


# ---- vertices --------------------------------------------------------------------------------------------------------
def core_number(G):
    """networkx.core_number on the GPU: {node: the largest k whose k-core holds the node}, Python ints."""
    _no_selfloops(G, _CORE_LOOPS)
    return _with_graph(G, lambda g: dict(zip(g.nodes, map(int, g.core_layers()[0]))))


def onion_layers(G):
    """networkx.onion_layers on the GPU: {node: the round of the peel in which the node leaves}, from 1."""
    _no_selfloops(G, _ONION_LOOPS)
    return _with_graph(G, lambda g: dict(zip(g.nodes, map(int, g.core_layers()[1]))))


def degeneracy(G):
    """The largest core number; 0 for the null graph."""
    _no_selfloops(G, _CORE_LOOPS)
    return _with_graph(G, lambda g: int(g.core_layers()[0].max()) if g.n else 0)


def _core_array(g, core_number):   # pylint: disable=redefined-outer-name
    """(n,) int64 core numbers in vertex order: the device pass, or the caller's dict keyed by node / (n,) array."""
    if core_number is None:
        return g.core_layers()[0].astype(np.int64)
    if isinstance(core_number, dict):
        return np.array([core_number[v] for v in g.nodes], dtype=np.int64).reshape(g.n)
    core = np.asarray(core_number, dtype=np.int64).ravel()
    if len(core) != g.n:
        raise ValueError(f"core_number must have {g.n} entries")
    return core


def _subgraph(g, keep, edges, return_vertices):
    """The package's graph type on the ascending vertex ids `keep` with `edges` already relabelled to 0 .. len(keep)-1."""
    adjacency = edges_to_adjacency(len(keep), edges)
    if not return_vertices:
        return adjacency
    nodes = g.nodes
    return adjacency, (keep if g.labels is None else [nodes[i] for i in keep])


def _core_subgraph(G, pick, k, core_number, return_vertices, below_max=0):   # pylint: disable=redefined-outer-name
    """networkx's _core_subgraph: the subgraph induced by the vertices pick(g, core, k) marks; k=None: the largest core
    number less below_max."""
    if core_number is None:
        _no_selfloops(G, _CORE_LOOPS)

    def run(g):
        core = _core_array(g, core_number)
        kk = max(core.tolist()) - below_max if k is None else k   # the null graph: max() raises, as in networkx
        keep = np.flatnonzero(pick(g, core, kk))
        return _subgraph(g, keep, _induced_edges(g, keep), return_vertices)
    return _with_graph(G, run)


def k_core(G, k=None, core_number=None, return_vertices=False):   # pylint: disable=redefined-outer-name
    """networkx.k_core on the GPU: the subgraph of the vertices of core number >= k (default: the largest)."""
    return _core_subgraph(G, lambda g, c, kk: c >= kk, k, core_number, return_vertices)


def k_shell(G, k=None, core_number=None, return_vertices=False):   # pylint: disable=redefined-outer-name
    """networkx.k_shell on the GPU: the subgraph of the vertices of core number == k (default: the largest)."""
    return _core_subgraph(G, lambda g, c, kk: c == kk, k, core_number, return_vertices)


def k_crust(G, k=None, core_number=None, return_vertices=False):   # pylint: disable=redefined-outer-name
    """networkx.k_crust on the GPU: the subgraph of the vertices of core number <= k (default: the largest less one)."""
    return _core_subgraph(G, lambda g, c, kk: c <= kk, k, core_number, return_vertices, below_max=1)


def k_corona(G, k, core_number=None, return_vertices=False):   # pylint: disable=redefined-outer-name
    """networkx.k_corona on the GPU: the subgraph of the vertices of core number k with exactly k neighbours in the
    k-core."""
    def pick(g, c, kk):
        inside = c >= kk
        u, v = g.edges[:, 0], g.edges[:, 1]
        in_core = np.bincount(u[inside[v]], minlength=g.n) + np.bincount(v[inside[u]], minlength=g.n)
        return (c == kk) & (in_core == kk)
    return _core_subgraph(G, pick, k, core_number, return_vertices)


# ---- edges -----------------------------------------------------------------------------------------------------------
def truss_number(G):
    """{(u, v): the largest k whose k-truss holds the edge}, Python ints, in canonical edge order (u before v in node
    order, sorted): an edge in t triangles of the k-truss has k <= t + 2, and an edge in no triangle has truss number 2."""
    _no_selfloops(G, _CORE_LOOPS)

    def run(g):
        nodes = g.nodes
        return {(nodes[u], nodes[v]): int(t) for (u, v), t in zip(g.edges.tolist(), g.truss_numbers())}
    return _with_graph(G, run)


def k_truss(G, k, return_vertices=False):
    """networkx.k_truss on the GPU: the subgraph of the edges that lie in at least k - 2 triangles of it -- the edges of
    truss number >= k -- without the vertices this leaves isolated."""
    _no_selfloops(G, _CORE_LOOPS)

    def run(g):
        edges = g.edges[g.truss_numbers() >= k]
        keep = np.unique(edges)
        new_id = np.full(g.n, -1, dtype=np.int64)
        new_id[keep] = np.arange(len(keep))
        return _subgraph(g, keep, new_id[edges], return_vertices)
    return _with_graph(G, run)
