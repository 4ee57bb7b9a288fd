"""Graph statistics without a GPU: the exported C ABI, the numpy restatement (tests/graphstats_reference.py) against
networkx on the graphs of tests/test_hip_graphstats.py, host-side argument checks, and the Python layer of
graphem-rapids_amd/graphstats.py over a stand-in handle that answers from the restatement."""
import ctypes
import os

import networkx as nx
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, graphstats

import graphstats_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATS_SYMBOLS = ["gh_cent_components", "gh_cent_distances", "gh_cent_triangles"]
PUBLIC = ["connected_components", "number_connected_components", "is_connected", "largest_connected_component",
          "eccentricity", "diameter", "radius", "average_shortest_path_length", "triangles", "clustering",
          "average_clustering", "transitivity", "graph_summary", "print_graph_summary"]


def test_graphstats_symbols_declared_exported_and_listed():
    from graphem_rapids_amd import build as gra_build
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    assert "graph statistics" in header
    gra_build.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in STATS_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name


def test_public_names_are_exported():
    for name in PUBLIC:
        assert name in gr.__all__, name
        assert getattr(gr, name) is getattr(graphstats, name)
    for name in ("component_labels", "distances", "triangle_counts"):
        assert callable(getattr(gr.CentralityGraph, name))
    for name in ("components", "distances", "triangles"):
        assert callable(getattr(_native.CentGraph, name))


# ---- the restatement equals networkx ---------------------------------------------------------------------------------
def _min_id_labels(G):
    want = np.zeros(G.number_of_nodes(), dtype=np.int32)
    for comp in nx.connected_components(G):
        want[list(comp)] = min(comp)
    return want


@pytest.mark.parametrize("name", ["gnp2000", "isolated", "path5000", "ws1000", "n1", "n2"])
def test_reference_labels_are_networkx_components(name):
    G = {"gnp2000": ref.gnp2000, "isolated": ref.isolated_plus_edge, "ws1000": ref.CONNECTED["ws1000"],
         "path5000": lambda: nx.from_edgelist(ref.permuted_path(5000).tolist()), "n1": ref.CONNECTED["n1"],
         "n2": ref.CONNECTED["n2"]}[name]()
    n = G.number_of_nodes()
    labels = ref.component_labels(n, ref.edge_array(G))
    assert np.array_equal(labels, _min_id_labels(G))
    if name == "gnp2000":
        assert len(np.unique(labels)) == 35 and np.bincount(labels).max() == 1965
    if name == "path5000":
        assert not labels.any()


@pytest.mark.parametrize("name", sorted(ref.CONNECTED))
def test_reference_distances_are_networkx(name):
    G = ref.CONNECTED[name]()
    n = G.number_of_nodes()
    src = np.arange(n) if n <= 300 else np.random.default_rng(0).integers(0, n, size=40)
    reached, dist_sum, ecc = ref.distances(n, ref.edge_array(G), src)
    for j, s in enumerate(src.tolist()):
        d = nx.single_source_shortest_path_length(G, s)
        assert (reached[j], dist_sum[j], ecc[j]) == (len(d), sum(d.values()), max(d.values()))
    if name == "ws1000":
        assert nx.diameter(G) == 11


def test_reference_distances_on_a_disconnected_graph():
    G = ref.gnp2000()
    src = [0, 5, 1999]
    reached, dist_sum, ecc = ref.distances(2000, ref.edge_array(G), src)
    for j, s in enumerate(src):
        d = nx.single_source_shortest_path_length(G, s)
        assert (reached[j], dist_sum[j], ecc[j]) == (len(d), sum(d.values()), max(d.values()))
        assert reached[j] < 2000


@pytest.mark.parametrize("name", sorted(ref.TRIANGLE_GRAPHS))
def test_reference_triangles_are_networkx(name):
    G = ref.TRIANGLE_GRAPHS[name]()
    n = G.number_of_nodes()
    t = ref.triangles(n, ref.edge_array(G))
    want = nx.triangles(G)
    assert t.tolist() == [want[v] for v in range(n)]
    if name == "k20":
        assert (t == 171).all()
    if name == "wheel5001":
        assert t[0] == 5000 and (t[1:] == 2).all()


def test_messy_edges_are_the_same_graph():
    G = ref.gnp2000()
    e = ref.edge_array(G)
    m = ref.messy(2000, e, seed=3)
    assert len(m) > len(e) and (m[:, 0] == m[:, 1]).any()
    assert np.array_equal(ref.canonical_edges(2000, m), ref.canonical_edges(2000, e))


# ---- host-side argument checks (nothing here reaches the device) -----------------------------------------------------
def test_weight_arguments_are_refused():
    G = nx.path_graph(4)
    for fn in (gr.eccentricity, gr.diameter, gr.radius, gr.average_shortest_path_length, gr.clustering,
               gr.average_clustering):
        with pytest.raises(NotImplementedError):
            fn(G, weight="weight")


def test_null_graph():
    G = nx.Graph()
    with pytest.raises(nx.NetworkXPointlessConcept, match="Connectivity is undefined for the null graph."):
        gr.is_connected(G)
    with pytest.raises(nx.NetworkXPointlessConcept, match="the null graph has no paths"):
        gr.average_shortest_path_length(G)
    for fn in (nx.is_connected, nx.average_shortest_path_length):   # the same messages as networkx's
        with pytest.raises(nx.NetworkXPointlessConcept) as theirs:
            fn(G)
        with pytest.raises(nx.NetworkXPointlessConcept) as ours:
            getattr(gr, fn.__name__)(G)
        assert str(ours.value) == str(theirs.value)
    assert gr.connected_components(G) == [] and gr.number_connected_components(G) == 0
    assert gr.triangles(G) == {} and gr.clustering(G) == {} and gr.eccentricity(G) == {}
    assert gr.transitivity(G) == 0
    assert gr.largest_connected_component(G).shape == (0, 0)
    s = gr.graph_summary(G)
    assert s["n_vertices"] == 0 and s["n_components"] == 0 and s["diameter"] is None
    g = gr.CentralityGraph(np.zeros((0, 2), dtype=np.int64))
    assert g.component_labels().shape == (0,) and g.triangle_counts().shape == (0,)
    assert [len(a) for a in g.distances()] == [0, 0, 0]


def test_bad_vertex_ids_are_refused_on_the_host():
    g = gr.CentralityGraph(np.zeros((0, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        g.distances([0])
    with pytest.raises(ValueError):
        g.distances([-1])
    with pytest.raises(ValueError):
        gr.eccentricity(g, v=3)
    with pytest.raises(ValueError):
        gr.triangles(g, nodes=[2])


# ---- the Python layer over a stand-in handle -------------------------------------------------------------------------
class _ReferenceHandle:
    """What _native.CentGraph offers the graph statistics, answered by the restatement."""

    def __init__(self, n, edges, device_id=0):
        del device_id
        self.n, self.e = int(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2)

    def components(self):
        labels = ref.component_labels(self.n, self.e)
        return labels, len(np.unique(labels))

    def distances(self, sources):
        return ref.distances(self.n, self.e, sources)

    def triangles(self):
        return ref.triangles(self.n, self.e)

    def close(self):
        pass


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(_native, "CentGraph", _ReferenceHandle)


def test_largest_component_tie_takes_the_smallest_member(host_only):
    G = nx.Graph([(0, 1), (1, 2), (3, 4), (5, 6), (6, 7)])
    assert max(nx.connected_components(G), key=len) == {0, 1, 2}
    adjacency, vertices = gr.largest_connected_component(G, return_vertices=True)
    assert set(vertices) == {0, 1, 2}
    assert adjacency.toarray().tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    # the later component larger: it wins; relabelled in ascending original id
    edges = np.array([[0, 1], [7, 3], [3, 5], [5, 9]])
    adjacency, vertices = gr.largest_connected_component(edges, return_vertices=True)
    assert list(vertices) == [3, 5, 7, 9]
    assert adjacency.toarray().tolist() == [[0, 1, 1, 0], [1, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]]
    assert adjacency.dtype == gr.edges_to_adjacency(2, [[0, 1]]).dtype


def test_python_layer_matches_networkx_on_labelled_nodes(host_only):
    G = nx.relabel_nodes(nx.barbell_graph(5, 2), {i: f"v{i}" for i in range(12)})
    assert gr.connected_components(G) == list(nx.connected_components(G))
    assert gr.is_connected(G) and gr.number_connected_components(G) == 1
    assert gr.eccentricity(G) == nx.eccentricity(G)
    assert gr.eccentricity(G, v="v3") == nx.eccentricity(G, v="v3")
    assert gr.eccentricity(G, v=["v3", "v6"]) == nx.eccentricity(G, v=["v3", "v6"])
    assert gr.diameter(G) == nx.diameter(G) and gr.radius(G) == nx.radius(G)
    assert gr.average_shortest_path_length(G) == nx.average_shortest_path_length(G)
    assert gr.triangles(G) == nx.triangles(G) and gr.triangles(G, "v0") == nx.triangles(G, "v0")
    assert all(isinstance(t, int) for t in gr.triangles(G).values())
    assert gr.clustering(G) == nx.clustering(G)
    assert gr.clustering(G, ["v4", "v5"]) == nx.clustering(G, ["v4", "v5"])
    assert gr.average_clustering(G) == nx.average_clustering(G)
    assert gr.average_clustering(G, count_zeros=False) == nx.average_clustering(G, count_zeros=False)
    assert gr.transitivity(G) == nx.transitivity(G)
    assert gr.average_shortest_path_length(nx.empty_graph(1)) == 0


def test_disconnected_graph_raises_networkx_messages(host_only):
    G = nx.Graph([(0, 1), (2, 3)])
    for fn in (gr.eccentricity, gr.diameter, gr.radius):
        with pytest.raises(nx.NetworkXError, match="^Found infinite path length because the graph is not connected$"):
            fn(G)
    with pytest.raises(nx.NetworkXError, match="^Graph is not connected.$"):
        gr.average_shortest_path_length(G)
    assert not gr.is_connected(G)


def test_print_graph_summary_wording(capsys):
    summary = {"n_vertices": 12345, "n_edges": 23456, "density": 0.000307842, "average_degree": 3.8001,
               "n_components": 1234, "largest_component_size": 10321, "diameter": 17,
               "average_shortest_path_length": 6.254, "average_clustering": 0.12345678}
    gr.print_graph_summary(summary)
    assert capsys.readouterr().out.splitlines() == [
        "Graph statistics:",
        "- Density: 0.000308",
        "- Average degree: 3.80",
        "- Number of connected components: 1,234",
        "- Largest component size: 10,321 vertices",
        "- Diameter: 17",
        "- Average shortest path length: 6.25",
        "- Average clustering coefficient: 0.1235",
    ]
    gr.print_graph_summary(dict(summary, diameter=None, average_shortest_path_length=None))
    out = capsys.readouterr().out.splitlines()
    assert out[5] == "- Diameter: Skipped" and out[6] == "- Average shortest path length: Skipped"
