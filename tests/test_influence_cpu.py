"""Influence layer without a GPU: the numpy restatement of the coin rule against closed forms, the CELF driver against
brute-force greedy, and graph input conversion."""
import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import graphem_rapids_amd as gr
from graphem_rapids_amd.influence import _graph_arcs, _ndlib_hops, celf_greedy

import ic_reference as ref


def _path(n):
    return np.column_stack([np.arange(n - 1), np.arange(1, n)])


@pytest.mark.parametrize("p,hops", [(0.5, None), (0.3, 3), (0.7, 5), (0.1, 1)])
def test_path_from_endpoint_closed_form(p, hops):
    n, T = 16, 4096
    t = ref.spread_trials(n, _path(n), False, [0], p, T, seed=123, max_hops=hops)
    q = ref.threshold(p) / 2 ** 24
    h = n - 1 if hops is None else hops
    mean = sum(q ** i for i in range(h + 1))
    se = t.std() / np.sqrt(T)
    assert abs(t.mean() - mean) <= 5 * se + 1e-12


def test_p0_and_hops0_give_seed_count():
    edges = gr.erdos_renyi_edges(300, 0.03, seed=1)
    seeds = [0, 5, 5, 17]
    assert (ref.spread_trials(300, edges, False, seeds, 0.0, 70, seed=2) == 3).all()
    assert (ref.spread_trials(300, edges, False, seeds, 0.9, 70, seed=2, max_hops=0) == 3).all()


def test_p1_gives_union_of_components():
    n = 400
    edges = gr.erdos_renyi_edges(n, 0.004, seed=3)
    _, lab = connected_components(gr.edges_to_adjacency(n, edges), directed=False)
    seeds = [1, 2, 399]
    want = np.isin(lab, lab[seeds]).sum()
    assert (ref.spread_trials(n, edges, False, seeds, 1.0, 65, seed=4) == want).all()


def test_coin_shared_by_both_directions():
    # an undirected edge given either way round is the same arc set, hence the same counts
    edges = gr.erdos_renyi_edges(200, 0.02, seed=5)
    a = ref.spread_trials(200, edges, False, [0, 1], 0.3, 100, seed=6)
    b = ref.spread_trials(200, edges[:, ::-1], False, [0, 1], 0.3, 100, seed=6)
    assert np.array_equal(a, b)


def _brute(f, n, k):
    seeds = []
    for _ in range(min(k, n)):
        base = f(seeds)
        best, bv = None, -1
        for v in range(n):
            if v in seeds:
                continue
            g = f(seeds + [v]) - base
            if g > bv:
                best, bv = v, g
        seeds.append(best)
    return seeds


@pytest.mark.parametrize("case", range(6))
def test_celf_equals_bruteforce_greedy(case):
    rng = np.random.default_rng(case)
    n = int(rng.integers(8, 61))
    k = int(rng.integers(1, 6))
    directed = case % 3 == 2
    arcs = np.column_stack([rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)])
    p, T, hops = [0.2, 0.5, 0.0, 0.35, 1.0, 0.1][case], 64, [None, 2, None, 1, None, 3][case]
    cache = {}

    def f(s):
        key = tuple(sorted(set(s)))
        if key not in cache:
            cache[key] = int(ref.spread_trials(n, arcs, directed, list(key), p, T, seed=case, max_hops=hops).sum())
        return cache[key]

    def evaluate(base, cand):
        b = f(base)
        return np.array([f(list(base) + [int(c)]) - b for c in cand], dtype=np.int64)

    want = _brute(f, n, k)
    for batch in (1, 3, 64):
        assert celf_greedy(evaluate, n, k, celf=True, batch=batch)[0] == want
    assert celf_greedy(evaluate, n, k, celf=False)[0] == want


def test_celf_ties_take_smallest_id():
    # every gain equal: plain greedy picks 0, 1, 2, ...
    seeds, evals = celf_greedy(lambda base, cand: np.zeros(len(cand), dtype=np.int64), 10, 4)
    assert seeds == [0, 1, 2, 3]
    # modular gains with ties: w[v]
    w = np.array([1, 3, 3, 0, 3, 2])
    seeds, _ = celf_greedy(lambda base, cand: w[np.asarray(cand)], 6, 5)
    assert seeds == [1, 2, 4, 5, 0]


def test_input_forms_give_the_same_arc_set():
    edges = np.array([[0, 1], [1, 0], [1, 2], [2, 2], [3, 1], [0, 1]])
    want = np.array([[0, 1], [1, 2], [1, 3]])
    G = nx.Graph()
    G.add_nodes_from(range(5))
    G.add_edges_from(edges.tolist())
    adj = sp.csr_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(5, 5))
    adj = adj + adj.T
    for graph, n in ((edges, 5), (G, None), (adj, None)):
        nn, arcs, directed, labels = _graph_arcs(graph, n)
        assert nn == 5 and not directed and labels is None
        assert np.array_equal(arcs, want)
    D = nx.DiGraph()
    D.add_edges_from(edges.tolist())
    nn, arcs, directed, _ = _graph_arcs(D)
    assert directed and np.array_equal(arcs, np.array([[0, 1], [1, 0], [1, 2], [3, 1]]))
    nn, arcs, directed, _ = _graph_arcs(edges, directed=True)
    assert directed and nn == 4 and np.array_equal(arcs, np.array([[0, 1], [1, 0], [1, 2], [3, 1]]))


def test_networkx_labels_are_mapped_in_node_order():
    G = nx.Graph([("a", "b"), ("b", "c")])
    n, arcs, _, labels = _graph_arcs(G)
    assert n == 3 and labels == ["a", "b", "c"] and np.array_equal(arcs, [[0, 1], [1, 2]])


def test_ndlib_iteration_mapping():
    assert _ndlib_hops(0) is None and _ndlib_hops(1) is None
    assert _ndlib_hops(2) == 0 and _ndlib_hops(200) == 198
