"""gh_ic_spread against the numpy restatement of its coin rule (tests/ic_reference.py), bit for bit per trial."""
import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
from graphem_rapids_amd.influence import InfluenceGraph, celf_greedy

import ic_reference as ref

pytestmark = pytest.mark.gpu


def _path(n):
    return np.column_stack([np.arange(n - 1), np.arange(1, n)])


def _star(n):
    return np.column_stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])


def _directed(n, m, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.integers(0, n, m), rng.integers(0, n, m)])


GRAPHS = {
    "path": (50, _path(50), False),
    "star": (300, _star(300), False),
    "er2000": (2000, gr.erdos_renyi_edges(2000, 0.004, seed=1), False),
    "rr5000": (5000, gr.random_regular_edges(5000, 8, seed=2), False),
    "planted": (3000, gr.planted_partition_edges(3000, 10, 6, 1, seed=3), False),
    "directed": (1500, _directed(1500, 6000, 4), True),
}


def _gpu(name, sets, p, T, hops, seed=7, base=None, budget=None):
    n, arcs, directed = GRAPHS[name]
    g = _native.ICGraph(n + 3, arcs, directed)   # three isolated vertices n .. n+2
    if budget is not None:
        g.set_memory_budget(budget)
    tot, tr = g.spread(sets, p, T, seed, -1 if hops is None else hops, base=base, per_trial=True)
    g.close()
    assert np.array_equal(tot, tr.sum(axis=1, dtype=np.int64))
    return tr


def _ref(name, s, p, T, hops, seed=7):
    n, arcs, directed = GRAPHS[name]
    return ref.spread_trials(n + 3, arcs, directed, s, p, T, seed, hops)


CASES = [  # (graph, p, n_trials, max_hops)
    ("path", 0.5, 1000, None), ("path", 0.3, 63, 3), ("path", 1.0, 65, 1), ("path", 0.0, 64, None),
    ("star", 0.3, 65, None), ("star", 0.05, 1, 1), ("star", 1.0, 64, 0),
    ("er2000", 0.3, 1000, None), ("er2000", 0.05, 63, 3), ("er2000", 1.0, 64, None), ("er2000", 0.0, 65, 1),
    ("rr5000", 0.05, 1000, None), ("rr5000", 0.3, 65, 3), ("rr5000", 1.0, 1, None), ("rr5000", 0.3, 64, 1),
    ("planted", 0.3, 1000, 3), ("planted", 0.05, 64, None), ("planted", 1.0, 63, 0),
    ("directed", 0.3, 1000, None), ("directed", 0.05, 65, 1), ("directed", 1.0, 64, 3), ("directed", 0.0, 1, None),
]


@pytest.mark.parametrize("name,p,T,hops", CASES)
def test_per_trial_counts_identical(name, p, T, hops):
    n = GRAPHS[name][0]
    sets = [[0], [], [1, 1, 5, 0, 5], [n, n + 1, 2], list(range(0, n, max(1, n // 7)))]
    got = _gpu(name, sets, p, T, hops)
    for s, row in zip(sets, got):
        assert np.array_equal(row, _ref(name, s, p, T, hops)), (name, s)


def test_invariance_edge_order_batching_chunking():
    n, arcs, _ = GRAPHS["er2000"]
    rng = np.random.default_rng(0)
    sets = [[i, (7 * i) % n] for i in range(0, 40)]
    a = _native.ICGraph(n, arcs)
    _, t0 = a.spread(sets, 0.3, 130, 11, -1, per_trial=True)
    shuffled = arcs[rng.permutation(len(arcs))][:, ::-1]
    shuffled = np.concatenate([shuffled, shuffled[:100], np.column_stack([np.arange(50), np.arange(50)])])
    b = _native.ICGraph(n, shuffled)
    assert b.arcs == a.arcs
    _, t1 = b.spread(sets, 0.3, 130, 11, -1, per_trial=True)
    assert np.array_equal(t0, t1)
    parts = [b.spread(sets[i:i + 7], 0.3, 130, 11, -1, per_trial=True)[1] for i in range(0, len(sets), 7)]
    assert np.array_equal(t0, np.concatenate(parts))
    b.set_memory_budget(1)   # one set per chunk
    assert np.array_equal(t0, b.spread(sets, 0.3, 130, 11, -1, per_trial=True)[1])
    a.close()
    b.close()


def test_chunk_state_regrown_kept_and_reused_across_budgets():
    """One handle, three calls: the chunk state is allocated for one seed set, re-grown for all 40, then reused as it is."""
    n, T = 200, 70   # 70 trials: two 64-bit words per entry
    rng = np.random.default_rng(5)
    arcs = np.concatenate([_path(n), rng.integers(0, n, (20, 2))])
    sets = [[5 * i] for i in range(40)]
    g = _native.ICGraph(n, arcs)
    # chunk state per seed set: n * (3 * 8 * W + 4 + 1 + 3 * 4) bytes with W = ceil(T / 64) words (vis, cur, nxt; the round
    # stamp, the touched byte and three lists per entry); sets per chunk = max(1, budget // that), at most the 40 there are
    per_set = n * (3 * 8 * 2 + 17)
    assert (1 << 30) // per_set >= 40
    runs = []
    for budget in (per_set, 0, per_set):   # 1 set per chunk, all 40 (0: the default, 1 GiB), 1 set in the larger state
        g.set_memory_budget(budget)
        runs.append(g.spread(sets, 0.3, T, 11, -1, per_trial=True)[1])
    g.close()
    assert runs[0].shape == (40, T) and runs[0].min() >= 1   # every seed counts itself
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("hops", [None, 2])
def test_marginal_mode(hops):
    n, arcs, _ = GRAPHS["planted"]
    g = _native.ICGraph(n, arcs)
    h = -1 if hops is None else hops
    base = [3, 10, 10, 77]
    cands = [[1], [3], [200], [], [5, 6]]
    _, marg = g.spread(cands, 0.2, 200, 5, h, base=base, per_trial=True)
    _, full = g.spread([base + c for c in cands], 0.2, 200, 5, h, per_trial=True)
    _, alone = g.spread([base], 0.2, 200, 5, h, per_trial=True)
    assert np.array_equal(marg, full - alone)
    g.close()


def test_scale_p1_random_regular_1m_equals_components():
    n = 1 << 20
    edges = gr.random_regular_edges(n, 8, seed=0)
    adj = gr.edges_to_adjacency(n, edges)
    _, lab = connected_components(adj, directed=False)
    seeds = [0, 12345, 999999]
    want = int(np.isin(lab, lab[seeds]).sum())
    g = _native.ICGraph(n, edges)
    _, tr = g.spread([seeds], 1.0, 130, 3, -1, per_trial=True)
    g.close()
    assert (tr[0] == want).all()


def _brute_greedy(name_or_graph, k, p, T, hops, seed):
    n, arcs, directed = name_or_graph
    cache = {}

    def f(s):
        key = tuple(sorted(set(s)))
        if key not in cache:
            cache[key] = int(ref.spread_trials(n, arcs, directed, list(key), p, T, seed, hops).sum())
        return cache[key]
    seeds = []
    for _ in range(k):
        base = f(seeds)
        gains = [f(seeds + [v]) - base if v not in seeds else -1 for v in range(n)]
        seeds.append(int(np.argmax(gains)))
    return seeds


def test_gpu_greedy_equals_bruteforce_restatement():
    n = 200
    edges = gr.erdos_renyi_edges(n, 0.02, seed=5)
    g = InfluenceGraph(edges, n=n)
    got, _ = g.greedy(4, p=0.2, n_trials=128, max_hops=None, seed=9)
    assert got == _brute_greedy((n, edges, False), 4, 0.2, 128, None, 9)
    g.close()


def test_gpu_celf_equals_plain_greedy():
    n = 5000
    g = InfluenceGraph(gr.random_regular_edges(n, 6, seed=8), n=n)
    a, ea = g.greedy(5, p=0.1, n_trials=64, max_hops=6, seed=3, celf=True)
    b, eb = g.greedy(5, p=0.1, n_trials=64, max_hops=6, seed=3, celf=False)
    assert a == b
    assert ea < eb
    g.close()


# the reference's tests/test_influence.py, restated
def test_reference_path():
    influence, iterations = gr.ndlib_estimated_influence(nx.path_graph(10), [0, 9], p=0.3, iterations_count=50)
    assert isinstance(influence, int) and isinstance(iterations, int)
    assert influence >= 2 and iterations == 50


def test_reference_probabilities():
    G = nx.complete_graph(8)
    vals = [gr.ndlib_estimated_influence(G, [0], p=p, iterations_count=30, n_trials=256, seed=1)[0] for p in (0.1, 0.5, 0.9)]
    assert vals[0] <= vals[1] <= vals[2]


def test_reference_empty_seed_set():
    assert gr.ndlib_estimated_influence(nx.path_graph(5), [], p=0.5, iterations_count=10)[0] == 0


def test_reference_disconnected():
    G = nx.Graph()
    G.add_edges_from([(0, 1), (1, 2), (3, 4), (4, 5)])
    influence, _ = gr.ndlib_estimated_influence(G, [0, 3], p=0.8, iterations_count=20)
    assert 2 <= influence <= 6


def test_ndlib_mapping_and_seed_from_numpy():
    G = nx.path_graph(12)
    assert gr.ndlib_estimated_influence(G, [0], p=1.0, iterations_count=5)[0] == 4   # hops <= 3
    assert gr.ndlib_estimated_influence(G, [0], p=1.0, iterations_count=1)[0] == 0
    np.random.seed(4)
    a = gr.ndlib_estimated_influence(G, [0, 6], p=0.5, n_trials=50)
    np.random.seed(4)
    assert gr.ndlib_estimated_influence(G, [0, 6], p=0.5, n_trials=50) == a


def test_readme_block():
    adjacency = gr.erdos_renyi_graph(n=1000, p=0.01)
    embedder = gr.create_graphem(adjacency, n_components=3)
    embedder.run_layout(num_iterations=5)
    seeds = gr.graphem_seed_selection(embedder, k=10)
    G = nx.from_scipy_sparse_array(adjacency)
    influence, _ = gr.ndlib_estimated_influence(G, seeds, p=0.1, iterations=100)
    assert 10 <= influence <= 1000
    greedy_seeds, total = gr.greedy_seed_selection(G, k=10, p=0.1)
    assert len(set(greedy_seeds)) == 10 and total > 0


def test_run_influence_benchmark_keys():
    res = gr.run_influence_benchmark(gr.planted_partition_edges, {"n": 600, "communities": 4, "deg_in": 6, "deg_out": 1},
                                     k=5, p=0.1, iterations=50, num_layout_iterations=5)
    keys = {"graph_type", "n", "m", "backend", "graphem_seeds", "greedy_seeds", "graphem_influence", "greedy_influence",
            "random_influence", "graphem_time", "greedy_time", "graphem_eval_time", "greedy_eval_time",
            "greedy_iterations", "graphem_norm_influence", "greedy_norm_influence", "random_norm_influence",
            "graphem_efficiency", "greedy_efficiency", "total_time"}
    assert keys <= set(res)
    assert res["n"] == 600 and len(res["greedy_seeds"]) == 5 and len(res["graphem_seeds"]) == 5


def test_invalid_arguments():
    g = _native.ICGraph(10, _path(10))
    for bad in (dict(p=1.5), dict(p=-0.1), dict(n_trials=0)):
        kw = dict(p=0.5, n_trials=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            g.spread([[0]], kw["p"], kw["n_trials"])
    with pytest.raises(ValueError):
        g.spread([[10]], 0.5, 8)
    with pytest.raises(ValueError):
        g.spread([[0]], 0.5, 8, base=[-1])
    g.close()
    with pytest.raises(ValueError):
        _native.ICGraph(10, [[0, 10]])
