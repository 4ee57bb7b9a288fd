"""The reference's eleven generator families without a GPU (graphem-rapids_amd/generators.py): signatures, closed forms against
networkx edge for edge, the library's host path against the restatement of the header's counter rules
(tests/generators_reference.py) bit for bit, the random geometric graph against networkx on our positions, the block model's
counts against the binomial law, and the sequential processes against networkx by invariants and by distribution.

Distribution checks (test_process_distribution_matches_networkx).  The statistic is two-sample, R = 10 graphs a side: the total
variation distance between the degree histograms in log2 bins (bin = floor(log2(degree + 1))) pooled over the seeds; for ws
and power_cluster also |difference of the mean average clustering|; for scale_free |difference of the mean edge count| / mean.
Its threshold is not a constant of this file: the test measures the same statistic networkx-against-networkx on 20 disjoint
pairs of seed sets, takes the largest value and allows 1.5 x that (20 splits sample the null only coarsely).  Measured null
maxima and thresholds (networkx 3.4.2; the run prints them with -s):

    family            statistic     null max    threshold   ours vs networkx
    ba                degree TV     0.0147      0.0220      0.0173
    ws                degree TV     0.0173      0.0260      0.0077
    ws                clustering    0.0172      0.0258      0.0062
    power_cluster     degree TV     0.0197      0.0295      0.0097
    power_cluster     clustering    0.0125      0.0187      0.0135
    scale_free        degree TV     0.0300      0.0450      0.0160
    scale_free        edge count    0.0504      0.0756      0.0064
    relaxed_caveman   degree TV     0.0070      0.0105      0.0000

(relaxed_caveman at l = k = 10: nearly every degree falls into the one bin 8 .. 15, so the histogram says little there; the
exact p = 0 invariant and the edge-count bound carry that family.)
"""
import inspect
import math

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import generators_reference as ref

# names and defaults of the reference's generators.py, copied by hand
REFERENCE_SIGNATURES = {
    "generate_sbm": [("n_per_block", 75), ("num_blocks", 4), ("p_in", 0.15), ("p_out", 0.01), ("labels", False), ("seed", 0)],
    "generate_ba": [("n", 300), ("m", 3), ("seed", 0)],
    "generate_ws": [("n", 1000), ("k", 6), ("p", 0.3), ("seed", 0)],
    "generate_power_cluster": [("n", 1000), ("m", 3), ("p", 0.5), ("seed", 0)],
    "generate_road_network": [("width", 30), ("height", 30)],
    "generate_bipartite_graph": [("n_top", 50), ("n_bottom", 100)],
    "generate_balanced_tree": [("r", 2), ("h", 10)],
    "generate_scale_free": [("n", 100), ("alpha", 0.41), ("beta", 0.54), ("gamma", 0.05), ("delta_in", 0.2), ("delta_out", 0),
                            ("seed", 0)],
    "generate_geometric": [("n", 100), ("radius", 0.2), ("dim", 2), ("seed", 0)],
    "generate_caveman": [("l", 10), ("k", 10)],
    "generate_relaxed_caveman": [("l", 10), ("k", 10), ("p", 0.1), ("seed", 0)],
}

GEN_SYMBOLS = ["gh_gen_create", "gh_gen_destroy", "gh_gen_last_error", "gh_gen_set_memory_budget", "gh_gen_sbm",
               "gh_gen_geometric", "gh_gen_ba", "gh_gen_edges", "gh_gen_positions"]

# the grids the host path here and the device (tests/test_hip_generators.py) are compared with the restatement on
_P5 = [[1.0, 0.5, 0.0, 0.2, 0.0], [0.5, 0.0, 0.0, 1.0, 0.3], [0.0, 0.0, 0.0, 0.0, 0.0], [0.2, 1.0, 0.0, 0.7, 1.0],
       [0.0, 0.3, 0.0, 1.0, 1.0]]
SBM_GRID = [
    ([75] * 4, (np.full((4, 4), 0.01) + np.eye(4) * 0.14).tolist(), 0),        # the reference's defaults
    ([5, 1, 0, 8, 2], _P5, 3),                                                 # p in {0, 1}, an empty block, a single vertex
    ([400], [[0.0001]], 7),                                                    # one block, several segments, tail redraws
    ([400], [[0.0]], 7),
    ([9], [[1.0]], 1),
    ([8], [[1.0]], 1),                                                         # even size: the diameters
    ([50, 100], [[0.0, 0.1], [0.1, 0.0]], 12345678901234567890),               # bipartite, a seed above 2^63
    ([300, 20, 130], [[0.02, 0.3, 0.004], [0.3, 0.9, 0.05], [0.004, 0.05, 0.1]], 2),
    ([], [], 0),
]
GEOMETRIC_GRID = [(100, 0.2, 2, 0), (300, 0.05, 1, 3), (257, 0.15, 3, 4), (200, 0.3, 5, 1), (120, 0.6, 8, 2),
                  (60, 1.0, 1, 5), (50, math.sqrt(2.0), 2, 6), (40, 3.0, 8, 7), (64, 0.0, 2, 8), (1, 0.5, 3, 9), (0, 0.5, 2, 9),
                  (500, 0.001, 2, 10), (400, 0.07, 3, 2 ** 64 - 1)]
BA_GRID = [(300, 3, 0), (50, 1, 1), (20, 19, 2), (100, 40, 3), (2, 1, 4), (500, 2, 2 ** 63 + 5), (64, 8, 6)]


@pytest.fixture(scope="module")
def host():
    g = _native.Generator(-1)
    yield g
    g.close()


def edge_set(graph):
    return sorted((min(u, v), max(u, v)) for u, v in graph.edges() if u != v)


def as_pairs(edges):
    return [tuple(e) for e in np.asarray(edges).tolist()]


def check_adjacency(adj, n):
    assert sp.issparse(adj) and adj.format == "csr" and adj.shape == (n, n)
    assert np.issubdtype(adj.dtype, np.integer)
    assert (adj != adj.T).nnz == 0
    assert adj.nnz == 0 or (adj.data == 1).all()
    assert adj.diagonal().sum() == 0


# ---- interface --------------------------------------------------------------------------------------------------------
def test_abi_symbols_are_bound():
    lib = _native.load()
    for name in GEN_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.SYMBOLS, name


@pytest.mark.parametrize("name", sorted(REFERENCE_SIGNATURES))
def test_reference_signature(name):
    assert name in gr.__all__
    params = inspect.signature(getattr(gr, name)).parameters
    positional = [(p.name, p.default) for p in params.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert positional == REFERENCE_SIGNATURES[name]
    extra = [p.name for p in params.values() if p.kind != p.POSITIONAL_OR_KEYWORD]
    assert extra == (["seed"] if name == "generate_bipartite_graph" else [])


@pytest.mark.parametrize("name", sorted(REFERENCE_SIGNATURES))
def test_defaults_give_a_symmetric_csr_of_ones(name):
    out = getattr(gr, name)()
    sizes = {"generate_sbm": 300, "generate_ba": 300, "generate_ws": 1000, "generate_power_cluster": 1000,
             "generate_road_network": 900, "generate_bipartite_graph": 150, "generate_balanced_tree": 2047,
             "generate_scale_free": 100, "generate_geometric": 100, "generate_caveman": 100, "generate_relaxed_caveman": 100}
    check_adjacency(out, sizes[name])
    assert out.nnz > 0


def test_sbm_labels():
    adj, labels = gr.generate_sbm(n_per_block=7, num_blocks=5, labels=True, seed=3)
    check_adjacency(adj, 35)
    assert np.array_equal(labels, np.repeat(np.arange(5), 7))
    assert (adj != gr.generate_sbm(n_per_block=7, num_blocks=5, seed=3)).nnz == 0


def test_edge_forms_are_sorted_int64():
    for edges in (gr.sbm_edges([30, 40], [[0.2, 0.1], [0.1, 0.3]], 1), gr.geometric_edges(200, 0.1, 2, 1),
                  gr.barabasi_albert_edges(100, 3, 1), gr.caveman_edges(3, 4), gr.road_network_edges(4, 5),
                  gr.balanced_tree_edges(3, 3), gr.watts_strogatz_edges(50, 4, 0.3, 1), gr.powerlaw_cluster_edges(60, 3, 0.5, 1),
                  gr.scale_free_edges(50, seed=1), gr.relaxed_caveman_edges(4, 5, 0.2, 1), gr.bipartite_edges(10, 20, 0.3, 1)):
        assert edges.dtype == np.int64 and edges.ndim == 2 and edges.shape[1] == 2 and len(edges) > 0
        assert (edges[:, 0] < edges[:, 1]).all()
        key = edges[:, 0] * (edges.max() + 1) + edges[:, 1]
        assert (np.diff(key) > 0).all()
    edges, pos = gr.geometric_edges(200, 0.1, 3, 1, return_positions=True)
    assert pos.shape == (200, 3) and pos.dtype == np.float32 and (pos >= 0).all() and (pos < 1).all()


def test_seeds():
    assert np.array_equal(gr.barabasi_albert_edges(200, 3, 5), gr.barabasi_albert_edges(200, 3, 5))
    assert not np.array_equal(gr.barabasi_albert_edges(200, 3, 5), gr.barabasi_albert_edges(200, 3, 6))
    assert not np.array_equal(gr.sbm_edges([100], [[0.1]], 0), gr.sbm_edges([100], [[0.1]], 1))
    assert not np.array_equal(gr.geometric_edges(100, 0.2, 2, 0), gr.geometric_edges(100, 0.2, 2, 1))
    a, b = gr.generate_bipartite_graph(seed=4), gr.generate_bipartite_graph(seed=4)
    assert (a != b).nnz == 0
    assert (gr.generate_bipartite_graph() != gr.generate_bipartite_graph()).nnz > 0      # unseeded: fresh seeds
    assert (gr.generate_bipartite_graph(20, 30, seed=1) != gr.edges_to_adjacency(50, gr.bipartite_edges(20, 30, 0.1, 1))).nnz == 0


def test_argument_errors():
    for call in (lambda: gr.generate_ba(10, 0), lambda: gr.generate_ba(10, 10), lambda: gr.generate_ws(10, 11, 0.1),
                 lambda: gr.generate_ws(10, 4, 1.5), lambda: gr.generate_power_cluster(10, 0, 0.5),
                 lambda: gr.generate_power_cluster(10, 11, 0.5), lambda: gr.generate_power_cluster(10, 3, -0.1),
                 lambda: gr.generate_scale_free(20, alpha=0.5, beta=0.3, gamma=0.1), lambda: gr.generate_scale_free(20, delta_in=-1),
                 lambda: gr.generate_scale_free(20, alpha=0, beta=0.95, gamma=0.05), lambda: gr.generate_relaxed_caveman(3, 4, 2.0),
                 lambda: gr.generate_geometric(10, 0.1, dim=9), lambda: gr.generate_geometric(10, 0.1, dim=0),
                 lambda: gr.generate_geometric(10, -0.1), lambda: gr.generate_sbm(p_in=1.5),
                 lambda: gr.sbm_edges([3, 4], [[0.1, 0.2], [0.3, 0.1]], 0), lambda: gr.sbm_edges([3, -4], [[0.1, 0.2], [0.2, 0.1]], 0),
                 lambda: gr.sbm_edges([3, 4], [[0.1]], 0), lambda: gr.balanced_tree_edges(0, 2)):
        with pytest.raises(ValueError):
            call()


# ---- closed forms: networkx edge for edge ---------------------------------------------------------------------------------
@pytest.mark.parametrize("l,k", [(1, 5), (4, 1), (3, 2), (10, 10), (7, 6), (1, 1)])
def test_caveman_is_networkx(l, k):
    assert as_pairs(gr.caveman_edges(l, k)) == edge_set(nx.caveman_graph(l, k))
    check_adjacency(gr.generate_caveman(l, k), l * k)


@pytest.mark.parametrize("width,height", [(1, 1), (1, 7), (6, 1), (2, 2), (5, 3), (30, 30), (4, 9)])
def test_road_network_is_networkx(width, height):
    G = nx.grid_2d_graph(width, height)
    G = nx.relabel_nodes(G, {node: i for i, node in enumerate(G.nodes())})      # as the reference relabels
    assert as_pairs(gr.road_network_edges(width, height)) == edge_set(G)
    check_adjacency(gr.generate_road_network(width, height), width * height)


@pytest.mark.parametrize("r,h", [(2, 0), (1, 4), (2, 1), (2, 10), (3, 4), (5, 2), (1, 0)])
def test_balanced_tree_is_networkx(r, h):
    G = nx.balanced_tree(r, h)
    assert as_pairs(gr.balanced_tree_edges(r, h)) == edge_set(G)
    check_adjacency(gr.generate_balanced_tree(r, h), G.number_of_nodes())


# ---- counter rules: host path == restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,P,seed", SBM_GRID)
def test_sbm_host_equals_restatement(host, sizes, P, seed):
    want = ref.sbm_edges(sizes, P, seed)
    assert np.array_equal(host.sbm(sizes, np.array(P, dtype=np.float64).reshape(len(sizes), len(sizes)), seed), want)
    n = int(sum(sizes))
    for a, (s, row) in enumerate(zip(sizes, P)):          # p = 0: none, p = 1: all
        off = int(sum(sizes[:a]))
        inside = int(((want[:, 0] >= off) & (want[:, 1] < off + s)).sum()) if len(want) else 0
        if row[a] == 0.0:
            assert inside == 0
        if row[a] == 1.0:
            assert inside == s * (s - 1) // 2
    assert len(want) == 0 or want.max() < n


@pytest.mark.parametrize("n,radius,dim,seed", GEOMETRIC_GRID)
def test_geometric_host_equals_restatement(host, n, radius, dim, seed):
    edges, pos = host.geometric(n, radius, dim, seed)
    want, want_pos = ref.geometric_edges(n, radius, dim, seed)
    assert np.array_equal(edges, want)
    assert np.array_equal(pos, want_pos)
    if radius >= math.sqrt(dim):
        assert len(edges) == n * (n - 1) // 2


@pytest.mark.parametrize("n,m,seed", BA_GRID)
def test_ba_host_equals_restatement(host, n, m, seed):
    edges = host.ba(n, m, seed)
    assert np.array_equal(edges, ref.ba_edges(n, m, seed))
    assert len(edges) == m * (n - m)
    assert host.rounds == 0


def test_public_edge_functions_are_the_rules():
    assert np.array_equal(gr.sbm_edges([40, 60], [[0.2, 0.05], [0.05, 0.1]], 9), ref.sbm_edges([40, 60], [[0.2, 0.05], [0.05, 0.1]], 9))
    assert np.array_equal(gr.geometric_edges(150, 0.12, 3, 9), ref.geometric_edges(150, 0.12, 3, 9)[0])
    assert np.array_equal(gr.barabasi_albert_edges(150, 4, 9), ref.ba_edges(150, 4, 9))
    adj = gr.generate_geometric(150, 0.12, 3, 9)
    assert np.array_equal(np.column_stack(sp.triu(adj, k=1).nonzero()), ref.geometric_edges(150, 0.12, 3, 9)[0])


# ---- geometric: the reference's own function on our positions --------------------------------------------------------------
@pytest.mark.parametrize("n,radius,dim,seed", [(300, 0.1, 2, 0), (200, 0.25, 3, 1), (150, 0.5, 5, 2), (100, 0.2, 1, 3),
                                               (120, 0.9, 8, 4)])
def test_geometric_is_networkx_on_our_positions(n, radius, dim, seed):
    edges, pos = gr.geometric_edges(n, radius, dim, seed, return_positions=True)
    p = pos.astype(np.float64)                                        # k / 2^24: exact
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)           # exact: at most 51 significant bits
    gap = np.abs(d2[np.triu_indices(n, 1)] - radius * radius).min()
    assert gap > 2.0 ** -40, "a pair sits on the boundary: choose other parameters"
    G = nx.random_geometric_graph(n, radius, dim=dim, pos={i: p[i].tolist() for i in range(n)})
    assert as_pairs(edges) == edge_set(G)


# ---- block model: the right distribution ------------------------------------------------------------------------------
def _binomial_bound(N, p):
    return 6.0 * math.sqrt(N * p * (1.0 - p)) + 1.0


@pytest.mark.parametrize("seed", [0, 1, 2, 12345])
def test_sbm_counts_follow_the_binomial_law(seed):
    sizes = [300, 500, 200, 41]
    P = np.array([[0.15, 0.01, 0.002, 0.5], [0.01, 0.05, 0.03, 0.0], [0.002, 0.03, 0.3, 1.0], [0.5, 0.0, 1.0, 0.9]])
    off = np.concatenate([[0], np.cumsum(sizes)])
    edges = gr.sbm_edges(sizes, P, seed)
    block = np.searchsorted(off, edges, side="right") - 1
    B = len(sizes)
    for a in range(B):
        mean = var = 0.0
        degree_sum = 0
        for b in range(B):
            N = sizes[a] * (sizes[a] - 1) // 2 if a == b else sizes[a] * sizes[b]
            X = int(((block[:, 0] == min(a, b)) & (block[:, 1] == max(a, b))).sum())
            p = P[a, b]
            if b >= a:
                print(f"seed {seed} blocks ({a}, {b}): {X} edges, N p = {N * p:.1f}, bound {_binomial_bound(N, p):.1f}")
                assert abs(X - N * p) <= _binomial_bound(N, p)
            w = 2 if a == b else 1                      # an inside edge adds 2 to the block's degree sum
            degree_sum += w * X
            mean += w * N * p
            var += w * w * N * p * (1.0 - p)
        assert abs(degree_sum - mean) <= 6.0 * math.sqrt(var) + 1.0


@pytest.mark.parametrize("seed", [0, 7])
def test_bipartite_has_no_edge_inside_a_side(seed):
    n_top, n_bottom = 50, 100
    adj = gr.generate_bipartite_graph(n_top, n_bottom, seed=seed)
    check_adjacency(adj, n_top + n_bottom)
    assert adj[:n_top, :n_top].nnz == 0 and adj[n_top:, n_top:].nnz == 0
    X = adj[:n_top, n_top:].nnz
    assert abs(X - n_top * n_bottom * 0.1) <= _binomial_bound(n_top * n_bottom, 0.1)


# ---- processes: invariants, first on networkx's output, then on ours --------------------------------------------------
def _ba_invariant(pairs, n, m):
    assert len(pairs) == m * (n - m)
    smaller = np.zeros(n, dtype=np.int64)
    for u, v in pairs:
        smaller[max(u, v)] += 1
    assert (smaller[m + 1:] == m).all()


@pytest.mark.parametrize("n,m,seed", [(300, 3, 0), (100, 1, 1), (60, 20, 2), (12, 11, 3)])
def test_ba_invariants(n, m, seed):
    _ba_invariant(edge_set(nx.barabasi_albert_graph(n, m, seed=seed)), n, m)
    _ba_invariant(as_pairs(gr.barabasi_albert_edges(n, m, seed)), n, m)
    check_adjacency(gr.generate_ba(n, m, seed), n)


@pytest.mark.parametrize("n,k,p,seed", [(200, 6, 0.3, 0), (50, 4, 1.0, 1), (31, 7, 0.5, 2), (20, 2, 0.9, 3), (12, 10, 0.8, 4)])
def test_ws_invariants(n, k, p, seed):
    ring = sorted((min(u, (u + j) % n), max(u, (u + j) % n)) for u in range(n) for j in range(1, k // 2 + 1))
    assert nx.watts_strogatz_graph(n, k, p, seed=seed).number_of_edges() == n * (k // 2)
    assert edge_set(nx.watts_strogatz_graph(n, k, 0.0, seed=seed)) == ring
    assert len(gr.watts_strogatz_edges(n, k, p, seed)) == n * (k // 2)
    assert as_pairs(gr.watts_strogatz_edges(n, k, 0.0, seed)) == ring
    assert as_pairs(gr.watts_strogatz_edges(n, n, p, seed)) == edge_set(nx.watts_strogatz_graph(n, n, p, seed=seed))   # complete


@pytest.mark.parametrize("l,k", [(10, 10), (3, 4), (1, 6)])
def test_relaxed_caveman_invariants(l, k):
    cave = edge_set(nx.caveman_graph(l, k))
    assert edge_set(nx.relaxed_caveman_graph(l, k, 0.0, seed=1)) == cave
    assert as_pairs(gr.relaxed_caveman_edges(l, k, 0.0, 1)) == cave
    assert len(edge_set(nx.relaxed_caveman_graph(l, k, 0.3, seed=1))) <= len(cave)      # a rewiring never adds an edge
    assert len(gr.relaxed_caveman_edges(l, k, 0.3, 1)) <= len(cave)


def test_power_cluster_and_scale_free_invariants():
    n, m = 200, 3
    for pairs in (edge_set(nx.powerlaw_cluster_graph(n, m, 0.5, seed=0)), as_pairs(gr.powerlaw_cluster_edges(n, m, 0.5, 0))):
        later = np.zeros(n, dtype=np.int64)
        for u, v in pairs:
            later[max(u, v)] += 1
        assert later[:m].sum() == 0 and (later[m:] >= 1).all() and (later[m:] <= m).all()      # every new vertex links back
    G = nx.scale_free_graph(80, seed=0)
    assert G.number_of_nodes() == 80 and gr.generate_scale_free(80, seed=0).shape == (80, 80)
    assert nx.scale_free_graph(2, seed=0).number_of_nodes() == 3 and gr.generate_scale_free(2, seed=0).shape == (3, 3)
    for pairs in (edge_set(G), as_pairs(gr.scale_free_edges(80, seed=0))):
        assert sorted(set(x for e in pairs for x in e)) == list(range(80))                      # nobody is isolated


# ---- processes: distribution against networkx, threshold from networkx against itself ----------------------------------
R = 10
SPLITS = 20


def _graph(pairs, n):
    G = nx.empty_graph(n)
    G.add_edges_from(pairs)
    return G


FAMILIES = {
    "ba": (lambda s: _graph(edge_set(nx.barabasi_albert_graph(300, 3, seed=s)), 300),
           lambda s: _graph(as_pairs(gr.barabasi_albert_edges(300, 3, s)), 300), ("degree",)),
    "ws": (lambda s: _graph(edge_set(nx.watts_strogatz_graph(300, 6, 0.3, seed=s)), 300),
           lambda s: _graph(as_pairs(gr.watts_strogatz_edges(300, 6, 0.3, s)), 300), ("degree", "clustering")),
    "power_cluster": (lambda s: _graph(edge_set(nx.powerlaw_cluster_graph(300, 3, 0.5, seed=s)), 300),
                      lambda s: _graph(as_pairs(gr.powerlaw_cluster_edges(300, 3, 0.5, s)), 300), ("degree", "clustering")),
    "scale_free": (lambda s: _graph(edge_set(nx.scale_free_graph(200, seed=s)), 200),
                   lambda s: _graph(as_pairs(gr.scale_free_edges(200, seed=s)), 200), ("degree", "edges")),
    "relaxed_caveman": (lambda s: _graph(edge_set(nx.relaxed_caveman_graph(10, 10, 0.1, seed=s)), 100),
                        lambda s: _graph(as_pairs(gr.relaxed_caveman_edges(10, 10, 0.1, s)), 100), ("degree",)),
}


def _summary(graphs):
    degrees = np.concatenate([[d for _, d in G.degree()] for G in graphs])
    hist = np.bincount(np.floor(np.log2(degrees + 1)).astype(np.int64), minlength=16).astype(np.float64)
    return {"degree": hist / hist.sum(), "clustering": float(np.mean([nx.average_clustering(G) for G in graphs])),
            "edges": float(np.mean([G.number_of_edges() for G in graphs]))}


def _statistic(a, b, kind):
    if kind == "degree":
        return 0.5 * float(np.abs(a["degree"] - b["degree"]).sum())
    if kind == "clustering":
        return abs(a["clustering"] - b["clustering"])
    return abs(a["edges"] - b["edges"]) / (0.5 * (a["edges"] + b["edges"]))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_process_distribution_matches_networkx(family):
    theirs, ours, kinds = FAMILIES[family]
    null = {kind: [] for kind in kinds}
    for split in range(SPLITS):                 # networkx against networkx on disjoint seed sets
        a = _summary([theirs(10_000 + 2 * R * split + i) for i in range(R)])
        b = _summary([theirs(10_000 + 2 * R * split + R + i) for i in range(R)])
        for kind in kinds:
            null[kind].append(_statistic(a, b, kind))
    a = _summary([ours(500 + i) for i in range(R)])
    b = _summary([theirs(700 + i) for i in range(R)])
    failures = []
    for kind in kinds:
        threshold = 1.5 * max(null[kind])
        value = _statistic(a, b, kind)
        print(f"{family} {kind}: null max {max(null[kind]):.4f}, threshold {threshold:.4f}, ours vs networkx {value:.4f}")
        if value > threshold:
            failures.append((kind, value, threshold))
    assert not failures
