"""Influence estimation and greedy seed selection: Monte Carlo Independent Cascade on the GPU.

The reference (graphem_rapids/influence.py, benchmark.py:246-379) scores seed sets with one pure-Python ndlib cascade and
selects greedy seeds with k * n of them.  Here every cascade runs in csrc/influence.hip (gh_ic_spread), thousands of
trials per call, with counter-based coins (include/graphem_hip.h): a result depends only on the arc set, the seed set,
p, max_hops, the number of trials and the seed, and tests/ic_reference.py recomputes it bit for bit in numpy.
"""
import heapq
import time

import numpy as np
import scipy.sparse as sp

from . import _native

_INT32_MAX = 2 ** 31 - 1


def _graph_arcs(graph, n=None, directed=None):
    """(n, (A, 2) int64 arcs, directed, labels): labels = the networkx node list when it is not 0 .. n-1, else None."""
    labels = None
    if hasattr(graph, "nodes") and hasattr(graph, "edges") and hasattr(graph, "is_directed"):   # networkx
        nodes = list(graph.nodes())
        if nodes != list(range(len(nodes))):
            labels = nodes
            index = {v: i for i, v in enumerate(nodes)}
            arcs = np.array([(index[u], index[v]) for u, v in graph.edges()], dtype=np.int64).reshape(-1, 2)
        else:
            arcs = np.array(list(graph.edges()), dtype=np.int64).reshape(-1, 2)
        n = len(nodes) if n is None else int(n)
        directed = graph.is_directed() if directed is None else bool(directed)
    elif sp.issparse(graph):   # this package's graph type: a (symmetric) adjacency matrix
        coo = sp.coo_matrix(graph)
        if coo.shape[0] != coo.shape[1]:
            raise ValueError(f"adjacency must be square, got {coo.shape}")
        keep = coo.data != 0
        arcs = np.column_stack([coo.row[keep], coo.col[keep]]).astype(np.int64)
        n = coo.shape[0] if n is None else int(n)
        directed = bool(directed)
    else:   # (E, 2) edge array
        arcs = np.asarray(graph, dtype=np.int64)
        if arcs.size == 0:
            arcs = arcs.reshape(0, 2)
        if arcs.ndim != 2 or arcs.shape[1] != 2:
            raise ValueError(f"an edge array must have shape (E, 2), got {arcs.shape}")
        n = (int(arcs.max()) + 1 if len(arcs) else 0) if n is None else int(n)
        directed = bool(directed)
    if len(arcs) and (arcs.min() < 0 or arcs.max() >= n):
        raise ValueError(f"edge endpoints must lie in [0, {n})")
    arcs = arcs[arcs[:, 0] != arcs[:, 1]]
    if not directed:
        arcs = np.sort(arcs, axis=1)
    arcs = np.unique(arcs, axis=0) if len(arcs) else arcs.reshape(0, 2)
    return n, arcs, directed, labels


def celf_greedy(evaluate, n, k, celf=True, batch=64):
    """Greedy maximisation of a monotone submodular set function over the vertices 0 .. n-1.

    evaluate(base, candidates) -> integer gains (len(candidates),): f(base + [c]) - f(base).  Each round takes the largest
    gain, the smallest vertex id among equal gains (the reference's strict '>' scan over range(n)).  celf: lazy greedy
    (CELF) -- stale gains are upper bounds; the stale tops of the heap are re-evaluated `batch` at a time (doubling while
    the top stays stale), and a top is accepted once it is fresh: every other entry then has a bound below its gain, or
    an equal bound and a larger id, so the choice is exactly plain greedy's.  Returns (seeds, evaluations)."""
    k = min(int(k), n)
    seeds, evals = [], 0
    if k <= 0:
        return seeds, evals
    if not celf:
        remaining = np.arange(n)
        for _ in range(k):
            gains = np.asarray(evaluate(list(seeds), remaining))
            evals += len(remaining)
            best = int(np.argmax(gains))          # first maximum = smallest id (remaining is ascending)
            seeds.append(int(remaining[best]))
            remaining = np.delete(remaining, best)
        return seeds, evals
    gains = np.asarray(evaluate([], np.arange(n)))
    evals += n
    heap = [(-int(g), v, 0) for v, g in enumerate(gains)]
    heapq.heapify(heap)
    for r in range(k):
        b = batch
        while heap[0][2] != r:
            stale = []
            while heap and heap[0][2] != r and len(stale) < b:
                stale.append(heapq.heappop(heap)[1])
            cand = np.array(stale, dtype=np.int64)
            fresh = np.asarray(evaluate(list(seeds), cand))
            evals += len(cand)
            for v, g in zip(stale, fresh):
                heapq.heappush(heap, (-int(g), v, r))
            b *= 2
        seeds.append(heapq.heappop(heap)[1])
    return seeds, evals


class InfluenceGraph:
    """One graph on the GPU for Independent Cascade estimates (gh_ic_create).

    graph: a networkx Graph / DiGraph, a scipy sparse adjacency (this package's graph type; undirected unless
    directed=True) or an (E, 2) edge array (undirected unless directed=True; n = largest id + 1 unless given).
    Self-loops are dropped and duplicate edges merged.  networkx node labels that are not 0 .. n-1 are mapped in node
    order; seeds are given and returned as labels."""

    def __init__(self, graph, n=None, directed=None, device_id=0):
        self.n, self.arcs, self.directed, self.labels = _graph_arcs(graph, n, directed)
        self._index = None if self.labels is None else {v: i for i, v in enumerate(self.labels)}
        self._ic = _native.ICGraph(max(self.n, 1), self.arcs, self.directed, device_id) if self.n > 0 else None

    def _ids(self, seeds):
        seeds = list(seeds)
        if self._index is not None:
            return np.array([self._index[s] for s in seeds], dtype=np.int64)
        ids = np.asarray(seeds, dtype=np.int64).ravel()
        if len(ids) and (ids.min() < 0 or ids.max() >= self.n):
            raise ValueError(f"seed ids must lie in [0, {self.n})")
        return ids

    @staticmethod
    def _hops(max_hops):
        if max_hops is None:
            return -1
        if max_hops < 0:
            raise ValueError("max_hops must be >= 0 or None")
        return min(int(max_hops), _INT32_MAX)

    def spread(self, seeds, p=0.1, n_trials=1024, max_hops=None, seed=0, return_trials=False):
        """Mean spread of the seed set over n_trials cascades (and the (n_trials,) per-trial counts with return_trials)."""
        ids = self._ids(seeds)
        if self._ic is None:
            trials = np.zeros(int(n_trials), dtype=np.int32)
        else:
            _, trials = self._ic.spread([ids], p, n_trials, seed, self._hops(max_hops), per_trial=True)
            trials = trials[0]
        mean = float(trials.sum(dtype=np.int64)) / int(n_trials)
        return (mean, trials) if return_trials else mean

    def marginal_totals(self, base, candidates, p, n_trials, max_hops=None, seed=0):
        """(len(candidates),) int64: sum over trials of |R(base + c)| - |R(base)|, the same coins for every candidate."""
        cand = np.asarray(candidates, dtype=np.int64).ravel()
        if self._ic is None or len(cand) == 0:
            return np.zeros(len(cand), dtype=np.int64)
        return self._ic.spread(cand.reshape(-1, 1), p, n_trials, seed, self._hops(max_hops),
                               base=np.asarray(base, dtype=np.int64))

    def greedy(self, k, p=0.1, n_trials=256, max_hops=None, seed=0, celf=True):
        """Greedy seeds maximising the sample-average spread over ONE fixed set of n_trials coin draws (common random
        numbers): (seeds, candidate evaluations)."""
        def evaluate(base, cand):
            return self.marginal_totals(base, cand, p, n_trials, max_hops, seed)
        seeds, evals = celf_greedy(evaluate, self.n, k, celf=celf)
        if self.labels is not None:
            seeds = [self.labels[s] for s in seeds]
        return seeds, evals

    def close(self):
        if self._ic is not None:
            self._ic.close()


def influence_spread(graph, seeds, p=0.1, n_trials=1024, max_hops=None, seed=0, return_trials=False):
    """Mean Independent Cascade spread of `seeds` over n_trials trials (duplicates allowed; an empty set gives 0).
    return_trials: also the (n_trials,) int32 spread of every trial."""
    g = graph if isinstance(graph, InfluenceGraph) else InfluenceGraph(graph)
    return g.spread(seeds, p, n_trials, max_hops, seed, return_trials)


def _ndlib_hops(iterations_count):
    """ndlib's iteration 0 returns the initial status and each later iteration moves that round's active vertices to
    state 2 ("removed"): after N iterations the removed vertices are those within N - 2 hops; none for N <= 1."""
    return None if iterations_count <= 1 else int(iterations_count) - 2


def _draw_seed(seed):
    return int(np.random.randint(0, 2 ** 62, dtype=np.int64)) if seed is None else int(seed)


def ndlib_estimated_influence(G, seeds, p=0.1, iterations_count=200, *, n_trials=1, seed=None, iterations=None):
    """The reference's call and return shape (influence.py:40-79): (vertices in ndlib state 2 after `iterations_count`
    iterations, iterations_count).  State 2 after N iterations = hop distance <= N - 2, 0 for N <= 1 (ndlib's documented
    iteration scheme; ndlib itself is not a dependency, so that off-by-one is the one point not checked against the
    package).  The reference sets the seeds' node configuration after set_initial_status, which its own test notes can
    leave 0 influenced; this implements what its docstring describes: the seeds start the cascade.

    n_trials = 1: an int from one cascade, as the reference; more: the float mean over n_trials cascades.
    seed = None draws the coin seed from numpy's global generator (np.random.seed makes a run reproducible).
    iterations: alias of iterations_count (the reference README's spelling)."""
    if iterations is not None:
        iterations_count = iterations
    iterations_count = int(iterations_count)
    seed = _draw_seed(seed)
    hops = _ndlib_hops(iterations_count)
    if hops is None:
        value = 0.0
    else:
        g = G if isinstance(G, InfluenceGraph) else InfluenceGraph(G)
        value = g.spread(seeds, p, n_trials, hops, seed)
    return (int(round(value)) if n_trials == 1 else float(value)), iterations_count


def greedy_seed_selection(G, k, p=0.1, iterations_count=200, *, n_trials=256, seed=None, celf=True):
    """The reference's greedy_seed_selection (influence.py:82-126): (seeds, total_iters), total_iters = candidate
    evaluations * iterations_count.  Objective: the spread summed over the SAME n_trials coin draws for every candidate
    (common random numbers), within iterations_count - 2 hops (ndlib_estimated_influence); gains compared as integer
    totals, ties to the smallest vertex id.  With fixed coins the objective is monotone submodular, so lazy greedy (CELF,
    celf=True) returns exactly what plain greedy (celf=False) returns, with far fewer evaluations."""
    seed = _draw_seed(seed)
    g = G if isinstance(G, InfluenceGraph) else InfluenceGraph(G)
    hops = _ndlib_hops(int(iterations_count))
    if hops is None:   # nothing is ever removed: every gain is 0, the reference picks 0, 1, 2, ...
        seeds, evals = celf_greedy(lambda base, cand: np.zeros(len(cand), dtype=np.int64), g.n, k, celf=celf)
        if g.labels is not None:
            seeds = [g.labels[s] for s in seeds]
    else:
        seeds, evals = g.greedy(k, p, n_trials, hops, seed, celf)
    return seeds, evals * int(iterations_count)


def run_influence_benchmark(graph_generator, graph_params, k=10, p=0.1, iterations=200, dim=3, num_layout_iterations=20,
                            layout_params=None, backend="hip"):
    """The reference's run_influence_benchmark (benchmark.py:246-379) on this package's embedder and the functions above:
    GraphEm seeds against greedy seeds and a random baseline, each scored with ndlib_estimated_influence.  The generator
    may return an (E, 2) edge array or an adjacency matrix.  Returns the reference's result keys."""
    from . import create_graphem, graphem_seed_selection, edges_to_adjacency
    start_time = time.time()
    out = graph_generator(**graph_params)
    if sp.issparse(out):
        adjacency = sp.csr_matrix(out)
        n = adjacency.shape[0]
        edges = np.column_stack(sp.triu(adjacency, k=1).nonzero()).astype(np.int64)
    else:
        edges = np.asarray(out, dtype=np.int64).reshape(-1, 2)
        n = max(int(edges.max()) + 1 if len(edges) else 0, int(graph_params.get("n", 0)))
        adjacency = edges_to_adjacency(n, edges)
    m = len(edges)
    if layout_params is None:
        layout_params = {"L_min": 10.0, "k_attr": 0.5, "k_inter": 0.1, "n_neighbors": 15, "sample_size": 512,
                         "batch_size": 1024}
    graph = InfluenceGraph(edges, n=n)
    embedder = create_graphem(adjacency, n_components=dim, backend=backend, verbose=False, **layout_params)

    graphem_start = time.time()
    graphem_seeds = graphem_seed_selection(embedder, k, num_iterations=num_layout_iterations)
    graphem_time = time.time() - graphem_start

    greedy_start = time.time()
    greedy_seeds, greedy_iters = greedy_seed_selection(graph, k, p, iterations)
    greedy_time = time.time() - greedy_start

    graphem_eval_start = time.time()
    graphem_influence, _ = ndlib_estimated_influence(graph, graphem_seeds, p, iterations)
    graphem_eval_time = time.time() - graphem_eval_start

    greedy_eval_start = time.time()
    greedy_influence, _ = ndlib_estimated_influence(graph, greedy_seeds, p, iterations)
    greedy_eval_time = time.time() - greedy_eval_start

    random_influences = []
    for _ in range(10):
        random_seeds = np.random.choice(n, k, replace=False)
        random_influences.append(ndlib_estimated_influence(graph, random_seeds, p, iterations)[0])
    random_influence = np.mean(random_influences)
    graph.close()

    results = {
        "graph_type": graph_generator.__name__,
        "n": n,
        "m": m,
        "backend": backend,
        "graphem_seeds": graphem_seeds,
        "greedy_seeds": greedy_seeds,
        "graphem_influence": graphem_influence,
        "greedy_influence": greedy_influence,
        "random_influence": random_influence,
        "graphem_time": graphem_time,
        "greedy_time": greedy_time,
        "graphem_eval_time": graphem_eval_time,
        "greedy_eval_time": greedy_eval_time,
        "greedy_iterations": greedy_iters,
        "graphem_norm_influence": graphem_influence / n,
        "greedy_norm_influence": greedy_influence / n,
        "random_norm_influence": random_influence / n,
    }
    results["graphem_efficiency"] = results["graphem_norm_influence"] / graphem_time if graphem_time > 0 else 0
    results["greedy_efficiency"] = results["greedy_norm_influence"] / greedy_time if greedy_time > 0 else 0
    results["total_time"] = time.time() - start_time
    return results
