"""Graph statistics on the GPU: what the reference's examples compute with networkx between loading a graph and embedding
it (real_world_datasets_example.py:111-175; random_regular_example.py and graph_generator_example.py print the same).

Connected components, eccentricity / diameter / radius / average shortest path length, triangles and the clustering
coefficients, under networkx's names and with networkx's results, plus largest_connected_component and graph_summary for
the example's analysis step.  The three passes are integer-exact HIP kernels over the centrality handle's CSR
(csrc/graphstats.hip: gh_cent_components, gh_cent_distances, gh_cent_triangles); the few divisions happen on the host,
one fp64 division of two exact integers each, which is what networkx's Python arithmetic does.

Every function takes what CentralityGraph takes -- a networkx Graph, a scipy sparse adjacency (this package's graph type),
an (E, 2) edge array or a CentralityGraph -- and results are keyed by node as the centrality drop-ins key theirs.
Undirected, unweighted graphs only.  Self-loops are dropped and duplicate edges merged.
"""
import numpy as np

from .centrality import CentralityGraph, _graph, _nx
from .generators import edges_to_adjacency

_NOT_CONNECTED = "Found infinite path length because the graph is not connected"


def _nx_error(msg):
    return _nx.NetworkXError(msg) if _nx is not None else ValueError(msg)


def _pointless(msg):
    return _nx.NetworkXPointlessConcept(msg) if _nx is not None else ValueError(msg)


def _unweighted(weight):
    if weight is not None:
        raise NotImplementedError("weighted graphs are not supported")


def _with_graph(G, fn):
    g, own = _graph(G)
    try:
        return fn(g)
    finally:
        if own:
            g.close()


# ---- components ------------------------------------------------------------------------------------------------------
def _components_of(labels):
    """The vertex-id arrays of the components that min-id `labels` describe, ordered by smallest member (each ascending)."""
    if len(labels) == 0:
        return []
    order = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    return np.split(order, cuts)


def connected_components(G):
    """networkx.connected_components on the GPU: a list of node sets ordered by smallest member (networkx's order for
    nodes in node order)."""
    def run(g):
        nodes = g.nodes
        return [{nodes[i] for i in comp} for comp in _components_of(g.component_labels())]
    return _with_graph(G, run)


def number_connected_components(G):
    """networkx.number_connected_components on the GPU."""
    return _with_graph(G, lambda g: len(np.unique(g.component_labels())))


def is_connected(G):
    """networkx.is_connected on the GPU; the null graph raises NetworkXPointlessConcept (ValueError without networkx)."""
    def run(g):
        if g.n == 0:
            raise _pointless("Connectivity is undefined for the null graph.")
        return not g.component_labels().any()   # one component: every label is vertex 0
    return _with_graph(G, run)


def _largest(comps):
    """Vertex ids (ascending) of the largest of _components_of's components; among equally large ones the one with the
    smallest member, which is what max(nx.connected_components(G), key=len) picks."""
    if not comps:
        return np.zeros(0, dtype=np.int64)
    return comps[int(np.argmax([len(c) for c in comps]))]   # argmax: the first of equal sizes


def _induced_edges(g, keep):
    """Edges of g among the ascending vertex ids `keep`, relabelled to 0 .. len(keep)-1 in that order."""
    new_id = np.full(g.n, -1, dtype=np.int64)
    new_id[keep] = np.arange(len(keep))
    e = new_id[g.edges]
    return e[(e >= 0).all(axis=1)]


def largest_connected_component(graph, return_vertices=False, n=None):
    """The largest connected component as this package's graph type (a symmetric CSR of ones), its vertices relabelled
    to 0 .. m-1 in ascending original id -- the reference example's G.subgraph(max(components, key=len)) followed by
    convert_node_labels_to_integers.  return_vertices=True: (adjacency, the original vertex ids (nodes for a labelled
    networkx graph)).  n: the vertex count of an (E, 2) edge array (default: largest id + 1)."""
    g, own = (graph, False) if isinstance(graph, CentralityGraph) else (CentralityGraph(graph, n=n), True)
    try:
        keep = _largest(_components_of(g.component_labels()))
        adjacency = edges_to_adjacency(len(keep), _induced_edges(g, keep))
        if not return_vertices:
            return adjacency
        nodes = g.nodes
        return adjacency, (keep if g.labels is None else [nodes[i] for i in keep])
    finally:
        if own:
            g.close()


# ---- distances -------------------------------------------------------------------------------------------------------
def _eccentricities(g, ids=None):
    reached, _, ecc = g.distances(ids)
    if (reached < g.n).any():
        raise _nx_error(_NOT_CONNECTED)
    return ecc


def eccentricity(G, v=None, sp=None, weight=None):
    """networkx.eccentricity on the GPU: a dict keyed by node; the value of node v when v is one node; the dict over
    the nodes of v when v is a collection.  A disconnected graph raises NetworkXError."""
    _unweighted(weight)
    if sp is not None:
        raise NotImplementedError("precomputed shortest paths are not supported")

    def run(g):
        nodes = g.nodes
        if v is None:
            return dict(zip(nodes, map(int, _eccentricities(g))))
        single = (v in g.labels) if g.labels is not None else np.ndim(v) == 0
        want = [v] if single else list(v)
        ecc = _eccentricities(g, g._ids(want))   # pylint: disable=protected-access
        return int(ecc[0]) if single else dict(zip(want, map(int, ecc)))
    return _with_graph(G, run)


def diameter(G, e=None, usebounds=False, weight=None):
    """networkx.diameter on the GPU: the largest eccentricity, from one all-sources pass."""
    _unweighted(weight)
    del usebounds   # a way to the same number
    if e is not None:
        return max(e.values())
    return int(_with_graph(G, _eccentricities).max())


def radius(G, e=None, usebounds=False, weight=None):
    """networkx.radius on the GPU: the smallest eccentricity, from one all-sources pass."""
    _unweighted(weight)
    del usebounds
    if e is not None:
        return min(e.values())
    return int(_with_graph(G, _eccentricities).min())


def _average_path_length(g):
    if g.n == 0:
        raise _pointless("the null graph has no paths, thus there is no average shortest path length")
    if g.n == 1:
        return 0
    reached, dist_sum, _ = g.distances()
    if (reached < g.n).any():
        raise _nx_error("Graph is not connected.")
    return int(dist_sum.sum()) / (g.n * (g.n - 1))   # exact integers, one division: networkx's value bit for bit


def average_shortest_path_length(G, weight=None, method=None):
    """networkx.average_shortest_path_length on the GPU: the integer sum of all hop distances over n (n - 1); 0 for one
    vertex.  A disconnected graph raises NetworkXError, the null graph NetworkXPointlessConcept."""
    _unweighted(weight)
    del method   # unweighted: breadth-first search whatever it names
    return _with_graph(G, _average_path_length)


# ---- triangles and clustering ----------------------------------------------------------------------------------------
def _select(g, values, nodes, convert):
    """values (n,) as networkx hands them out: a dict over all nodes, one value for one node, a dict over a collection."""
    if nodes is None:
        return dict(zip(g.nodes, map(convert, values)))
    single = (nodes in g.labels) if g.labels is not None else np.ndim(nodes) == 0
    want = [nodes] if single else list(nodes)
    picked = [convert(values[i]) for i in g._ids(want)]   # pylint: disable=protected-access
    return picked[0] if single else dict(zip(want, picked))


def _clustering_values(g):
    """(n,) float64: 2 t / (d (d - 1)), 0 for d < 2 -- one fp64 division of two exact integers per vertex."""
    t, d = g.triangle_counts(), g.degree()
    pairs = d * (d - 1)
    out = np.zeros(g.n)
    ok = pairs > 0
    out[ok] = (2 * t[ok]).astype(np.float64) / pairs[ok].astype(np.float64)
    return out


def triangles(G, nodes=None):
    """networkx.triangles on the GPU: ints, keyed by node (one int for one node)."""
    return _with_graph(G, lambda g: _select(g, g.triangle_counts(), nodes, int))


def clustering(G, nodes=None, weight=None):
    """networkx.clustering on the GPU: 2 t / (d (d - 1)) per node, 0 for a degree below 2."""
    _unweighted(weight)
    return _with_graph(G, lambda g: _select(g, _clustering_values(g), nodes, float))


def _average_clustering(g, count_zeros=True):
    c = [float(x) for x in _clustering_values(g)]
    if not count_zeros:
        c = [x for x in c if abs(x) > 0]
    return sum(c) / len(c)   # networkx's sum, in node order


def average_clustering(G, nodes=None, weight=None, count_zeros=True):
    """networkx.average_clustering on the GPU (every node): the mean of clustering(G), without its zeros when
    count_zeros=False.  The null graph raises ZeroDivisionError, as in networkx."""
    _unweighted(weight)
    if nodes is not None:
        c = list(clustering(G, list(nodes)).values())
        if not count_zeros:
            c = [x for x in c if abs(x) > 0]
        return sum(c) / len(c)
    return _with_graph(G, lambda g: _average_clustering(g, count_zeros))


def transitivity(G):
    """networkx.transitivity on the GPU: the integer sum of 2 t over the integer sum of d (d - 1); 0 without triangles."""
    def run(g):
        t, d = g.triangle_counts(), g.degree()
        closed = 2 * int(t.sum())
        return 0 if closed == 0 else closed / int((d * (d - 1)).sum())
    return _with_graph(G, run)


# ---- the example's analysis step -------------------------------------------------------------------------------------
def graph_summary(graph, path_stats=True, n=None):
    """The statistics the reference example prints before it embeds a graph (real_world_datasets_example.py:120-170), as a
    dict: n_vertices, n_edges, density, average_degree, n_components, largest_component_size, and for the largest
    component diameter, average_shortest_path_length and average_clustering.

    path_stats=False leaves diameter and average_shortest_path_length None.  There is no size cut-off (the reference
    skips both from 10 000 vertices on): the all-sources pass holds three n / 64-word bit rows per source group and
    costs n^2 / 64 words per breadth-first level, so it is the caller who decides whether a graph is too large for it.
    n: the vertex count of an (E, 2) edge array (default: largest id + 1)."""
    g, own = (graph, False) if isinstance(graph, CentralityGraph) else (CentralityGraph(graph, n=n), True)
    try:
        nv, ne = g.n, len(g.edges)
        comps = _components_of(g.component_labels())
        keep = _largest(comps)
        out = {
            "n_vertices": nv,
            "n_edges": ne,
            "density": 2 * ne / (nv * (nv - 1)) if nv > 1 else 0,
            "average_degree": 2 * ne / nv if nv > 0 else 0,
            "n_components": len(comps),
            "largest_component_size": len(keep),
            "diameter": None,
            "average_shortest_path_length": None,
            "average_clustering": None,
        }
        if nv == 0:
            return out
        cc = g if len(keep) == nv else CentralityGraph(_induced_edges(g, keep), n=len(keep), device_id=g.device_id)
        try:
            if path_stats:
                reached, dist_sum, ecc = cc.distances()
                assert (reached == cc.n).all(), "the largest component is connected"
                out["diameter"] = int(ecc.max())
                out["average_shortest_path_length"] = int(dist_sum.sum()) / (cc.n * (cc.n - 1)) if cc.n > 1 else 0
            out["average_clustering"] = _average_clustering(cc)
        finally:
            if cc is not g:
                cc.close()
        return out
    finally:
        if own:
            g.close()


def print_graph_summary(summary):
    """Print a graph_summary dict in the wording of the reference example's "Graph statistics:" block."""
    print("Graph statistics:")
    print(f"- Density: {summary['density']:.6f}")
    print(f"- Average degree: {summary['average_degree']:.2f}")
    print(f"- Number of connected components: {summary['n_components']:,}")
    print(f"- Largest component size: {summary['largest_component_size']:,} vertices")
    if summary.get("diameter") is not None:
        print(f"- Diameter: {summary['diameter']}")
    else:
        print("- Diameter: Skipped")
    if summary.get("average_shortest_path_length") is not None:
        print(f"- Average shortest path length: {summary['average_shortest_path_length']:.2f}")
    else:
        print("- Average shortest path length: Skipped")
    if summary.get("average_clustering") is not None:
        print(f"- Average clustering coefficient: {summary['average_clustering']:.4f}")
