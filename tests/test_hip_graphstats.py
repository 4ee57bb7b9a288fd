"""gh_cent_components / gh_cent_distances / gh_cent_triangles (csrc/graphstats.hip) and graphem-rapids_amd/graphstats.py
against networkx, against scipy.sparse.csgraph where networkx's per-vertex search is slow, against the numpy restatement
(tests/graphstats_reference.py), and against itself (identical integers across budgets and edge order).  Every expected
value is an integer or one division of two, so every comparison is exact."""
import functools

import networkx as nx
import numpy as np
import pytest
from scipy.sparse.csgraph import connected_components as sp_components
from scipy.sparse.csgraph import shortest_path

import graphem_rapids_amd as gr

import graphstats_reference as ref

pytestmark = pytest.mark.gpu


def _adjacency(G):
    """Rows in node order, the vertex order of CentralityGraph (barbell_graph's nodes are not 0 .. n-1 in order)."""
    return nx.to_scipy_sparse_array(G, nodelist=list(G), format="csr")


@functools.lru_cache(maxsize=None)
def _gnp():
    G = ref.gnp2000()
    comps = list(nx.connected_components(G))
    return G, comps, ref.edge_array(G)


@functools.lru_cache(maxsize=None)
def _hops(name):
    """(G, (n, n) hop distances) of a connected case: scipy's breadth-first search, checked against networkx's
    diameter where that is quick."""
    G = ref.CONNECTED[name]()
    n = G.number_of_nodes()
    D = shortest_path(_adjacency(G), method="D", unweighted=True) if n > 1 else np.zeros((1, 1))
    assert np.isfinite(D).all()
    return G, D.astype(np.int64)


# ---- components ------------------------------------------------------------------------------------------------------
def test_components_permuted_path_is_one_component():
    edges = ref.permuted_path(5000, seed=0)
    g = gr.CentralityGraph(edges, n=5000)
    labels = g.component_labels()
    g.close()
    assert labels.dtype == np.int32 and labels.shape == (5000,)
    assert not labels.any()
    assert gr.is_connected(edges) and gr.number_connected_components(edges) == 1


def test_components_gnp_labels_and_largest_component():
    G, comps, edges = _gnp()
    assert len(comps) == 35 and max(map(len, comps)) == 1965   # the fixture is what the issue says it is
    g = gr.CentralityGraph(G)
    labels = g.component_labels()
    assert np.array_equal(labels, ref.component_labels(2000, edges))
    assert len(np.unique(labels)) == sp_components(_adjacency(G), directed=False)[0] == 35
    assert gr.connected_components(g) == comps
    assert gr.number_connected_components(g) == 35 and not gr.is_connected(g)
    adjacency, vertices = gr.largest_connected_component(g, return_vertices=True)
    g.close()
    largest = max(comps, key=len)
    assert list(vertices) == sorted(largest)
    want = nx.convert_node_labels_to_integers(G.subgraph(largest), ordering="sorted")
    want = nx.to_scipy_sparse_array(want, nodelist=range(len(largest)), format="csr")
    assert adjacency.shape == want.shape and (adjacency != want).nnz == 0
    assert (adjacency.data == 1).all()


def test_components_isolated_vertices_and_one_edge():
    G = ref.isolated_plus_edge()
    labels = gr.CentralityGraph(G).component_labels()
    want = np.arange(302)
    want[301] = 17
    assert np.array_equal(labels, want)
    assert gr.number_connected_components(G) == 301
    assert gr.connected_components(G) == list(nx.connected_components(G))
    adjacency, vertices = gr.largest_connected_component(G, return_vertices=True)
    assert list(vertices) == [17, 301] and adjacency.toarray().tolist() == [[0, 1], [1, 0]]


def test_components_of_tiny_graphs():
    assert gr.connected_components(nx.Graph()) == []
    assert gr.connected_components(nx.empty_graph(1)) == [{0}]
    assert gr.connected_components(nx.empty_graph(2)) == [{0}, {1}]
    assert gr.connected_components(nx.path_graph(2)) == [{0, 1}]
    assert gr.is_connected(nx.empty_graph(1)) and not gr.is_connected(nx.empty_graph(2))
    assert gr.CentralityGraph(nx.path_graph(2)).component_labels().tolist() == [0, 0]


def test_components_do_not_depend_on_edge_order_duplicates_or_loops():
    _, _, edges = _gnp()
    want = ref.component_labels(2000, edges)
    for seed in (1, 2):
        got = gr.CentralityGraph(ref.messy(2000, edges, seed), n=2000).component_labels()
        assert np.array_equal(got, want)


# ---- distances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.CONNECTED))
def test_distances_all_sources(name):
    G, D = _hops(name)
    n = G.number_of_nodes()
    g = gr.CentralityGraph(G)
    reached, dist_sum, ecc = g.distances()
    assert reached.dtype == np.int64 and dist_sum.dtype == np.int64 and ecc.dtype == np.int32
    assert (reached == n).all()
    assert np.array_equal(dist_sum, D.sum(axis=1))
    assert np.array_equal(ecc, D.max(axis=1))
    assert gr.eccentricity(g) == dict(zip(G, D.max(axis=1).tolist()))
    assert gr.eccentricity(g, v=list(G)[-1]) == D[-1].max()
    assert gr.diameter(g) == D.max() and gr.radius(g) == D.max(axis=1).min()
    want = int(D.sum()) / (n * (n - 1)) if n > 1 else 0
    assert gr.average_shortest_path_length(g) == want
    g.close()
    if n <= 400:   # networkx itself, where it is quick
        assert gr.eccentricity(G) == nx.eccentricity(G)
        assert gr.diameter(G) == nx.diameter(G) and gr.radius(G) == nx.radius(G)
        assert gr.average_shortest_path_length(G) == nx.average_shortest_path_length(G)
    if name == "ws1000":
        assert gr.diameter(G) == 11


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_distances_source_lists_with_repeats(count):
    G, D = _hops("grid30")
    src = np.random.default_rng(count).integers(0, 900, size=count)
    src[-1] = src[0]   # a repeat, also for count > 1 within and across groups
    if count > 64:
        src[64] = src[3]
    reached, dist_sum, ecc = gr.CentralityGraph(G).distances(src)
    want = ref.distances(900, ref.edge_array(G), src)
    assert np.array_equal(reached, want[0]) and np.array_equal(dist_sum, want[1]) and np.array_equal(ecc, want[2])
    assert np.array_equal(dist_sum, D[src].sum(axis=1))


def test_distances_on_a_disconnected_graph():
    G, comps, edges = _gnp()
    g = gr.CentralityGraph(G)
    reached, dist_sum, ecc = g.distances()
    assert (reached < 2000).all()
    size = np.zeros(2000, dtype=np.int64)
    for comp in comps:
        size[list(comp)] = len(comp)
    assert np.array_equal(reached, size)
    D = shortest_path(_adjacency(G), method="D", unweighted=True)
    finite = np.where(np.isfinite(D), D, 0).astype(np.int64)
    assert np.array_equal(dist_sum, finite.sum(axis=1)) and np.array_equal(ecc, finite.max(axis=1))
    src = [0, 7, 7, 1999]
    want = ref.distances(2000, edges, src)
    got = g.distances(src)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for fn in (gr.diameter, gr.radius, gr.eccentricity):
        with pytest.raises(nx.NetworkXError, match="^Found infinite path length because the graph is not connected$"):
            fn(g)
    with pytest.raises(nx.NetworkXError, match="^Graph is not connected.$"):
        gr.average_shortest_path_length(g)
    g.close()


def test_distances_do_not_depend_on_the_memory_budget():
    G, _ = _hops("ws1000")
    g = gr.CentralityGraph(G)
    default = g.distances()
    g.set_memory_budget(1)   # one 64-source group at a time
    one = g.distances()
    g.set_memory_budget(3 * 24 * 1000)   # three groups: batches of 3, 3, .., 1
    three = g.distances()
    g.close()
    for a, b, c in zip(default, one, three):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_distances_long_path():
    n = 3000   # 2999 levels: far above the flag check interval and any flag array sized for small diameters
    g = gr.CentralityGraph(nx.path_graph(n))
    src = np.array([0, n - 1, n // 2, 1])
    reached, dist_sum, ecc = g.distances(src)
    g.close()
    assert reached.tolist() == [n] * 4
    assert ecc.tolist() == [n - 1, n - 1, n // 2, n - 2]
    tri = lambda k: k * (k + 1) // 2   # 1 + 2 + .. + k
    assert dist_sum.tolist() == [tri(n - 1), tri(n - 1), tri(n // 2) + tri(n - 1 - n // 2), 1 + tri(n - 2)]


def test_distances_refuse_bad_ids_and_accept_nothing():
    g = gr.CentralityGraph(nx.path_graph(5))
    assert [len(a) for a in g.distances([])] == [0, 0, 0]
    with pytest.raises(ValueError):
        g.distances([5])
    with pytest.raises(ValueError):
        g._g.distances([-1])
    only = g._g.distances([0, 4], reached=False, dist_sum=False)
    assert only[0] is None and only[1] is None and only[2].tolist() == [4, 4]
    g.close()


# ---- triangles and clustering ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.TRIANGLE_GRAPHS))
def test_triangles_and_clustering(name):
    G = ref.TRIANGLE_GRAPHS[name]()
    n = G.number_of_nodes()
    g = gr.CentralityGraph(G)
    t = g.triangle_counts()
    assert t.dtype == np.int64
    want = nx.triangles(G)
    assert t.tolist() == [want[v] for v in G]
    if name == "k20":
        assert (t == 171).all()
    if name == "star300":
        assert not t.any()
    if name == "wheel5001":
        assert t[0] == 5000 and (t[1:] == 2).all()
    assert gr.triangles(g) == want and gr.triangles(g, 0) == want[0]
    assert gr.clustering(g) == nx.clustering(G)
    assert gr.transitivity(g) == nx.transitivity(G)
    assert abs(gr.average_clustering(g) - nx.average_clustering(G)) <= n * 2.0 ** -52
    if t.any():   # without a triangle both divide by zero
        assert abs(gr.average_clustering(g, count_zeros=False) - nx.average_clustering(G, count_zeros=False)) <= n * 2.0 ** -52
    g.close()


def test_triangles_do_not_depend_on_edge_order_duplicates_or_loops():
    G = ref.TRIANGLE_GRAPHS["ba1000"]()
    edges = ref.edge_array(G)
    want = gr.CentralityGraph(G).triangle_counts()
    assert np.array_equal(want, ref.triangles(1000, edges))
    for seed in (1, 2):
        assert np.array_equal(gr.CentralityGraph(ref.messy(1000, edges, seed), n=1000).triangle_counts(), want)


# ---- the example's analysis step -------------------------------------------------------------------------------------
def test_graph_summary_is_the_reference_examples_analysis():
    G, comps, _ = _gnp()
    n, m = G.number_of_nodes(), G.number_of_edges()
    largest = max(comps, key=len)
    G_cc = nx.convert_node_labels_to_integers(G.subgraph(largest).copy())
    want = {
        "n_vertices": n,
        "n_edges": m,
        "density": 2 * m / (n * (n - 1)),
        "average_degree": 2 * m / n,
        "n_components": len(comps),
        "largest_component_size": len(largest),
        "diameter": nx.diameter(G_cc),
        "average_shortest_path_length": nx.average_shortest_path_length(G_cc),
        "average_clustering": nx.average_clustering(G_cc),
    }
    got = gr.graph_summary(G)
    assert set(got) == set(want)
    for key, value in want.items():
        assert got[key] == value, key   # average_clustering too: the same terms, summed in the same (node) order
    quick = gr.graph_summary(_adjacency(G), path_stats=False)
    assert quick["diameter"] is None and quick["average_shortest_path_length"] is None
    assert {k: v for k, v in quick.items() if v is not None} == {k: got[k] for k, v in quick.items() if v is not None}


def test_snap_file_to_embedder_as_the_readme_shows(tmp_path):
    G, comps, edges = _gnp()
    path = tmp_path / "disconnected.txt"
    rows = "".join(f"{7 * u + 10}\t{7 * v + 10}\n" for u, v in edges.tolist())   # labels that are not 0 .. n-1
    path.write_text("# a disconnected SNAP edge list\n" + rows, encoding="utf-8")
    vertices, snap_edges = gr.load_snap_edge_list(str(path))
    assert len(vertices) == len({int(x) for x in edges.ravel()})   # isolated vertices do not occur in an edge list
    adjacency, kept = gr.largest_connected_component(snap_edges, return_vertices=True, n=len(vertices))
    assert adjacency.shape == (1965, 1965) and adjacency.nnz == 2 * G.subgraph(max(comps, key=len)).number_of_edges()
    summary = gr.graph_summary(adjacency)
    assert summary["n_components"] == 1 and summary["largest_component_size"] == 1965
    assert summary["diameter"] == gr.graph_summary(G)["diameter"]
    embedder = gr.create_graphem(adjacency, n_components=2, backend="hip", verbose=False, seed=0)
    positions = np.asarray(embedder.run_layout(num_iterations=2))
    assert positions.shape == (1965, 2) and np.isfinite(positions).all()
