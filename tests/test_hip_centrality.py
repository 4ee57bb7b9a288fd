"""gh_cent_* (csrc/centrality.hip) against networkx, against the numpy restatement (tests/centrality_reference.py) where
networkx is too slow, and against itself (bitwise invariance across budgets, edge order and runs)."""
import functools

import networkx as nx
import numpy as np
import pytest
from scipy import stats
from scipy.sparse.csgraph import shortest_path

import graphem_rapids_amd as gr
from graphem_rapids_amd import centrality as cent

import centrality_reference as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL, ATOL_EIG = 1e-9, 1e-12, 1e-8


def _nx_from_edges(n, edges):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(np.asarray(edges).tolist())
    return G


GRAPHS = {
    "path50": lambda: nx.path_graph(50),
    "star300": lambda: nx.star_graph(299),
    "cycle101": lambda: nx.cycle_graph(101),
    "grid30": lambda: nx.convert_node_labels_to_integers(nx.grid_2d_graph(30, 30)),
    "k20": lambda: nx.complete_graph(20),
    "barbell": lambda: nx.barbell_graph(20, 1),   # (a longer bridge leaves the Perron root within 1e-10 of the next)
    "ba1000": lambda: nx.barabasi_albert_graph(1000, 3, seed=1),
    "ws1000": lambda: nx.connected_watts_strogatz_graph(1000, 6, 0.1, seed=2),
    "rr2000": lambda: _nx_from_edges(2000, gr.random_regular_edges(2000, 8, seed=3)),
    "planted3000": lambda: _nx_from_edges(3000, gr.planted_partition_edges(3000, 10, 6, 1, seed=3)),
    "er2000": lambda: _nx_from_edges(2000, gr.erdos_renyi_edges(2000, 0.004, seed=1)),
    "n1": lambda: nx.empty_graph(1),
    "n2": lambda: nx.path_graph(2),
    "odd130": lambda: nx.random_labeled_tree(130, seed=5) if hasattr(nx, "random_labeled_tree") else nx.random_tree(130, seed=5),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    G = GRAPHS[name]()
    n = G.number_of_nodes()
    want = {
        "betweenness": nx.betweenness_centrality(G),
        "load": nx.load_centrality(G),
        "closeness": nx.closeness_centrality(G),
        "pagerank": nx.pagerank(G),
    }
    try:
        want["eigenvector"] = nx.eigenvector_centrality_numpy(G)
    except nx.AmbiguousSolution:
        want["eigenvector"] = None
    except TypeError:   # n <= 2: scipy's eigs refuses k >= n - 1; the dense Perron vector instead
        w, V = np.linalg.eigh(nx.to_numpy_array(G))
        v = V[:, -1]
        want["eigenvector"] = dict(zip(G.nodes(), v / (np.sign(v.sum()) * np.linalg.norm(v))))
    nodes = list(G.nodes())   # CentralityGraph returns arrays in node order (barbell_graph's is not 0 .. n-1)
    return G, {k: (None if v is None else np.array([v[i] for i in nodes])) for k, v in want.items()}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_against_networkx(name):
    G, want = _case(name)
    g = cent.CentralityGraph(G)
    got = g.paths()
    for key in ("betweenness", "load", "closeness"):
        np.testing.assert_allclose(got[key], want[key], rtol=RTOL, atol=ATOL, err_msg=key)
    # the single-measure methods compute the same numbers
    np.testing.assert_array_equal(g.betweenness(), got["betweenness"])
    np.testing.assert_array_equal(g.load(), got["load"])
    np.testing.assert_array_equal(g.closeness(), got["closeness"])
    np.testing.assert_allclose(g.pagerank(), want["pagerank"], rtol=RTOL, atol=ATOL)
    if want["eigenvector"] is None:
        with pytest.raises(nx.AmbiguousSolution):
            g.eigenvector()
    else:
        np.testing.assert_allclose(g.eigenvector(), want["eigenvector"], rtol=0, atol=ATOL_EIG)
    np.testing.assert_array_equal(g.degree(), [d for _, d in G.degree()])
    g.close()


def test_drop_in_functions_return_dicts_keyed_by_label():
    G = nx.relabel_nodes(nx.barbell_graph(6, 3), lambda v: f"n{v}")
    for ours, theirs, tol in [(gr.betweenness_centrality, nx.betweenness_centrality, ATOL),
                              (gr.load_centrality, nx.load_centrality, ATOL),
                              (gr.closeness_centrality, nx.closeness_centrality, ATOL),
                              (gr.pagerank, nx.pagerank, ATOL),
                              (gr.eigenvector_centrality_numpy, nx.eigenvector_centrality_numpy, ATOL_EIG)]:
        a, b = ours(G), theirs(G)
        assert list(a) == list(b)
        np.testing.assert_allclose([a[k] for k in b], [b[k] for k in b], rtol=RTOL if tol == ATOL else 0, atol=tol)
    assert gr.closeness_centrality(G, u="n3") == pytest.approx(nx.closeness_centrality(G, u="n3"), rel=1e-12)
    assert gr.load_centrality(G, v="n7") == pytest.approx(nx.load_centrality(G, v="n7"), rel=1e-9)
    with pytest.raises(nx.AmbiguousSolution):
        gr.eigenvector_centrality_numpy(nx.Graph([(0, 1), (2, 3)]))


@pytest.mark.parametrize("seed", [0, 1, 42])
def test_sampled_betweenness_equals_networkx(seed):
    G, _ = _case("ba1000")
    want = nx.betweenness_centrality(G, k=100, seed=seed)
    g = cent.CentralityGraph(G)
    np.testing.assert_allclose(g.betweenness(k=100, seed=seed), [want[i] for i in range(1000)], rtol=RTOL, atol=ATOL)
    got = gr.betweenness_centrality(G, k=100, seed=seed)
    np.testing.assert_allclose([got[i] for i in range(1000)], [want[i] for i in range(1000)], rtol=RTOL, atol=ATOL)
    g.close()


def _raw(g, sources):
    return g.raw_paths(sources, True, True, True)


def test_bitwise_across_budgets_edge_order_and_runs():
    n = 2000
    edges = gr.random_regular_edges(n, 8, seed=3)
    src = np.random.default_rng(0).permutation(n)[:1000]   # 16 groups, the last one short
    g = cent.CentralityGraph(edges, n=n)
    base = _raw(g, src)
    per_group = n * (32 * 64 + 32)
    for budget in (1, per_group, 3 * per_group, 7 * per_group, 1 << 40, 0):
        g.set_memory_budget(budget)
        for a, b in zip(base, _raw(g, src)):
            assert np.array_equal(a, b), budget
    again = _raw(g, src)
    for a, b in zip(base, again):
        assert np.array_equal(a, b)
    g.close()
    rng = np.random.default_rng(1)
    messy = np.concatenate([edges[:, ::-1], edges[:300], np.column_stack([np.arange(50), np.arange(50)])])
    messy = messy[rng.permutation(len(messy))]
    h = cent.CentralityGraph(messy, n=n)
    assert h._g.edges == len(edges)
    for a, b in zip(base, _raw(h, src)):
        assert np.array_equal(a, b)
    x1, x2 = h.pagerank(), cent.CentralityGraph(edges, n=n).pagerank()
    assert np.array_equal(x1, x2)
    h.close()


def test_path_state_regrown_kept_and_reused_across_budgets():
    """One handle, three calls: the path state is allocated for one group, re-grown for all five, then reused as it is."""
    from graphem_rapids_amd import _native
    n = 300
    g = _native.CentGraph(n, gr.erdos_renyi_edges(n, 0.03, seed=1))
    src = np.arange(n)   # 5 groups of 64 sources, the last one short
    # path state per 64-source group: n * (64 * (4 + 8 + 4 + 8 + 8) + 3 * 8 + 8) bytes (dist, sigma, npred, delta, lam per
    # entry; vis, cur, nxt and the level range per word); groups per batch = max(1, budget // that), at most the 5 there are
    per_group = n * (64 * 32 + 32)
    assert (1 << 30) // per_group >= 5
    runs = []
    for budget in (per_group, 0, per_group):   # 1 group, all 5 (0: the default, 1 GiB), 1 group in the larger state
        g.set_memory_budget(budget)
        runs.append(g.paths(src))
    g.close()
    assert runs[0][2].min() >= 1   # every source reached itself: the call did run
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_exact_paths_20000_against_restatement():
    n = 20000
    edges = gr.random_regular_edges(n, 3, seed=7)
    g = cent.CentralityGraph(edges, n=n)
    bc, ld, reached, dsum = _raw(g, np.arange(n))
    # closeness inputs of every source against scipy's breadth-first search
    for s0 in range(0, n, 2000):
        d = shortest_path(ref.adjacency(n, edges), unweighted=True, indices=np.arange(s0, s0 + 2000))
        fin = np.isfinite(d)
        np.testing.assert_array_equal(reached[s0:s0 + 2000], fin.sum(axis=1))
        np.testing.assert_array_equal(dsum[s0:s0 + 2000], np.where(fin, d, 0).sum(axis=1).astype(np.int64))
    want_total = float((dsum - (reached - 1)).sum())
    assert abs(bc.sum() - want_total) <= 1e-9 * want_total
    assert abs(ld.sum() - want_total) <= 1e-9 * want_total
    # the dependencies themselves, over 320 sources that span five groups, against the restatement
    src = np.random.default_rng(2).permutation(n)[:320]
    got = _raw(g, src)
    want = ref.paths(n, edges, src, batch=160)
    for a, b in zip(got[:2], want[:2]):
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)
    for a, b in zip(got[2:], want[2:]):
        np.testing.assert_array_equal(a, b)
    g.close()


def test_sampled_paths_at_a_million_vertices():
    n = 1_000_000
    edges = gr.random_regular_edges(n, 3, seed=11)
    g = cent.CentralityGraph(edges, n=n)
    src = np.array(cent.sample_sources(range(n), 64, 5))
    bc, ld, reached, dsum = _raw(g, src)
    want_total = float((dsum - (reached - 1)).sum())
    assert abs(bc.sum() - want_total) <= 1e-9 * want_total
    assert abs(ld.sum() - want_total) <= 1e-9 * want_total
    for s in src[:2]:   # the identity per source
        b1, l1, r1, d1 = _raw(g, [s])
        w = float(d1[0] - (r1[0] - 1))
        assert abs(b1.sum() - w) <= 1e-9 * w and abs(l1.sum() - w) <= 1e-9 * w
    pick = [0, 31, 63]
    d = shortest_path(ref.adjacency(n, edges), unweighted=True, indices=src[pick])
    fin = np.isfinite(d)
    np.testing.assert_array_equal(reached[pick], fin.sum(axis=1))
    np.testing.assert_array_equal(dsum[pick], np.where(fin, d, 0).sum(axis=1).astype(np.int64))
    g.close()


@pytest.mark.parametrize("name", ["path50", "star300", "grid30", "ba1000", "er2000"])
def test_pagerank_iterations_match_restatement(name):
    G, _ = _case(name)
    n = G.number_of_nodes()
    edges = np.array(G.edges()).reshape(-1, 2)
    g = cent.CentralityGraph(G)
    for alpha, tol in [(0.85, 1e-6), (0.5, 1e-9), (0.99, 1e-8)]:
        x, its = g._g.pagerank(alpha, 1000, tol)   # raw: -1 when 1000 iterations do not converge
        xr, itr = ref.pagerank(n, edges, alpha, 1000, tol)
        assert its == itr
        np.testing.assert_allclose(x, xr, rtol=RTOL, atol=ATOL)
    x, its = g.pagerank(0.85, 1000, 1e-8, return_iterations=True)
    if its > 3:
        with pytest.raises(nx.PowerIterationFailedConvergence):
            g.pagerank(0.85, its - 1, 1e-8)
    with pytest.raises(nx.PowerIterationFailedConvergence):
        gr.pagerank(G, max_iter=1, tol=0.0)
    g.close()


def _small_generator(n=400, d=4, seed=1):
    return gr.random_regular_edges(n, d, seed=seed)


def _two_parts(n=300):
    e = gr.random_regular_edges(n // 2, 4, seed=2)
    return np.concatenate([e, e + n // 2])


@pytest.mark.parametrize("gen,params", [(_small_generator, {"n": 400}), (_two_parts, {"n": 300}),
                                        (gr.generate_random_regular, {"n": 256, "d": 3, "seed": 4})])
def test_benchmark_functions(gen, params):
    res = gr.benchmark_correlations(gen, params, num_iterations=5, sample_size=64, n_neighbors=5, seed=0)
    keys = ["n", "m", "density", "avg_degree", "layout_time", "graph_type", "n_components", "backend", "radii",
            "positions", "degree", "betweenness", "eigenvector", "pagerank", "closeness", "node_load", "total_time"]
    for k in keys + ["correlations", "centrality_time"]:
        assert k in res, k
    n = res["n"]
    edges = gen(**params)
    if hasattr(edges, "tocoo"):
        G = nx.from_scipy_sparse_array(edges)
        G.remove_edges_from(nx.selfloop_edges(G))
    else:
        G = _nx_from_edges(n, edges)
    arr = lambda d: np.array([d[i] for i in range(n)])   # noqa: E731
    np.testing.assert_allclose(res["betweenness"], arr(nx.betweenness_centrality(G)), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(res["node_load"], arr(nx.load_centrality(G)), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(res["closeness"], arr(nx.closeness_centrality(G)), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(res["pagerank"], arr(nx.pagerank(G)), rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(res["degree"], [d for _, d in G.degree()])
    if nx.is_connected(G):
        np.testing.assert_allclose(res["eigenvector"], arr(nx.eigenvector_centrality_numpy(G)), rtol=0, atol=ATOL_EIG)
    else:
        np.testing.assert_allclose(res["eigenvector"], arr(nx.degree_centrality(G)), rtol=RTOL, atol=ATOL)
    assert res["positions"].shape == (n, 2) and res["radii"].shape == (n,)
    for name in cent.CORRELATION_KEYS:
        rho, p = stats.spearmanr(res["radii"], res[name])
        c = res["correlations"][name]
        assert (np.isnan(rho) and np.isnan(c["rho"])) or c["rho"] == rho
        assert (np.isnan(p) and np.isnan(c["p"])) or c["p"] == p
    sampled = gr.run_benchmark(gen, params, num_iterations=3, sample_size=64, n_neighbors=5, seed=0, betweenness_k=50)
    src = cent.sample_sources(range(n), 50, 0)
    bc, ld, _, _ = ref.paths(n, np.array(G.edges()).reshape(-1, 2), src)
    np.testing.assert_allclose(sampled["betweenness"], bc * cent.betweenness_scale(n, True, 50), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sampled["closeness"], res["closeness"], rtol=0, atol=0)
    assert sampled["betweenness_k"] == 50
