"""Centrality measures on the GPU, and the reference's run_benchmark / benchmark_correlations on top of them.

The reference (graphem_rapids/benchmark.py:18-243) computes six centralities with networkx before it times the layout:
betweenness, load and closeness each run one pure-Python breadth-first search per vertex, PageRank and eigenvector
centrality are scipy iterations on the host.  Here one all-sources pass in csrc/centrality.hip (gh_cent_paths) yields
betweenness, load and closeness together, PageRank iterates on the device (gh_cent_pagerank), and the eigenvector solve
is the Lanczos iteration of spectral.py on the adjacency SpMV gh_spmv_adj_shift.  Normalisation stays on the host,
as networkx does it (_rescale, newman_betweenness_centrality, closeness_centrality).

Undirected, unweighted graphs only.  Self-loops are dropped and duplicate edges merged.
"""
import logging
import random
import time

import numpy as np
import scipy.sparse as sp

from . import _native
from .influence import _graph_arcs

logger = logging.getLogger(__name__)

try:   # networkx is optional; its exception types are used when it is there
    import networkx as _nx
except ImportError:   # pragma: no cover
    _nx = None


def _ambiguous(msg):
    return _nx.AmbiguousSolution(msg) if _nx is not None else ValueError(msg)


def _no_convergence(iterations):
    if _nx is not None:
        return _nx.PowerIterationFailedConvergence(iterations)
    return RuntimeError(f"power iteration failed to converge within {iterations} iterations")


def sample_sources(nodes, k, seed=None):
    """networkx's choice of k sources for sampled betweenness: seed.sample(list(G.nodes()), k), seed an int (a fresh
    random.Random), a random.Random, or None (the random module's global generator)."""
    nodes = list(nodes)
    if seed is None:
        rng = random._inst   # pylint: disable=protected-access  (what networkx's py_random_state(None) hands out)
    elif isinstance(seed, random.Random):
        rng = seed
    else:
        rng = random.Random(seed)
    return rng.sample(nodes, int(k))


def betweenness_scale(n, normalized, k=None):
    """networkx _rescale for an undirected graph without endpoints: the factor the raw sums are multiplied by (None:
    left as they are)."""
    if normalized:
        scale = None if n <= 2 else 1 / ((n - 1) * (n - 2))
    else:
        scale = 0.5
    if scale is not None and k is not None:
        scale = scale * n / k
    return scale


def closeness_from(reached, dist_sum, n, wf_improved=True):
    """networkx closeness_centrality from the reached count (source included) and distance sum of every source."""
    reached = np.asarray(reached, dtype=np.float64)
    tot = np.asarray(dist_sum, dtype=np.float64)
    out = np.zeros(len(reached))
    ok = (tot > 0) & (n > 1)
    out[ok] = (reached[ok] - 1.0) / tot[ok]
    if wf_improved:
        out[ok] *= (reached[ok] - 1.0) / (n - 1)
    return out


class CentralityGraph:
    """One undirected graph on the GPU for centrality measures (gh_cent_create).

    graph: a networkx Graph, a scipy sparse adjacency (this package's graph type) or an (E, 2) edge array (n = largest id
    + 1 unless given).  networkx node labels that are not 0 .. n-1 are mapped in node order; arrays are returned in that
    vertex order.  Directed input raises NotImplementedError."""

    def __init__(self, graph, n=None, device_id=0):
        if hasattr(graph, "is_directed") and graph.is_directed():
            raise NotImplementedError("centrality measures here are for undirected graphs")
        if hasattr(graph, "is_multigraph") and graph.is_multigraph():
            raise NotImplementedError("multigraphs are not supported")
        self.n, self.edges, _, self.labels = _graph_arcs(graph, n, False)
        self.device_id = int(device_id)
        self._g = _native.CentGraph(self.n, self.edges, self.device_id) if self.n > 0 else None

    # ---- helpers ----------------------------------------------------------------------------------------------------
    @property
    def nodes(self):
        return list(range(self.n)) if self.labels is None else list(self.labels)

    def _ids(self, vertices):
        vertices = list(vertices)
        if self.labels is not None:
            index = {v: i for i, v in enumerate(self.labels)}
            return np.array([index[v] for v in vertices], dtype=np.int64)
        ids = np.asarray(vertices, dtype=np.int64).ravel()
        if len(ids) and (ids.min() < 0 or ids.max() >= self.n):
            raise ValueError(f"vertex ids must lie in [0, {self.n})")
        return ids

    def as_dict(self, values):
        return dict(zip(self.nodes, map(float, values)))

    def set_memory_budget(self, nbytes):
        """Device bytes of path state a shortest-path pass may hold (0: the default, 1 GiB).  Results do not depend
        on it."""
        if int(nbytes) < 0:
            raise ValueError("the memory budget must be >= 0 (0: the default)")
        if self._g is not None:
            self._g.set_memory_budget(int(nbytes))

    def raw_paths(self, sources, betweenness=True, load=True, distances=True):
        """gh_cent_paths over vertex ids `sources`: (raw betweenness (n,), raw load (n,), reached (S,), dist_sum (S,))."""
        src = np.asarray(sources, dtype=np.int64).ravel()
        if len(src) and (src.min() < 0 or src.max() >= self.n):
            raise ValueError(f"source ids must lie in [0, {self.n})")
        if self._g is None:
            z = np.zeros(0)
            return (z if betweenness else None, z if load else None,
                    np.zeros(len(src), np.int64) if distances else None, np.zeros(len(src), np.int64) if distances else None)
        return self._g.paths(src, betweenness, load, distances)

    def _sampled(self, k, seed, sources):
        if sources is not None:
            if k is not None:
                raise ValueError("give k or sources, not both")
            return self._ids(sources), None
        if k is None:
            return np.arange(self.n, dtype=np.int64), None
        k = int(k)
        if k < 0 or k > self.n:
            raise ValueError(f"k must lie in [0, {self.n}]")
        return self._ids(sample_sources(self.nodes, k, seed)), k

    # ---- measures ---------------------------------------------------------------------------------------------------
    def degree(self):
        """(n,) int64 vertex degrees (self-loops dropped, duplicate edges merged)."""
        return np.bincount(self.edges.ravel(), minlength=self.n).astype(np.int64)

    def betweenness(self, normalized=True, k=None, seed=None, sources=None):
        """networkx betweenness_centrality(G, k, normalized, seed=seed): with k, sources = networkx's sample and the sums
        scaled by n / k.  sources: an explicit source list instead (scaled by n / len(sources) as well)."""
        src, k_used = self._sampled(k, seed, sources)
        if sources is not None:
            k_used = len(src)
        bc, _, _, _ = self.raw_paths(src, True, False, False)
        scale = betweenness_scale(self.n, normalized, k_used)
        return bc * scale if scale is not None else bc

    def load(self, normalized=True):
        """networkx load_centrality(G, normalized=normalized)."""
        _, ld, _, _ = self.raw_paths(np.arange(self.n), False, True, False)
        if normalized and self.n > 2:
            ld = ld * (1.0 / ((self.n - 1) * (self.n - 2)))
        return ld

    def closeness(self, wf_improved=True):
        """networkx closeness_centrality(G, wf_improved=wf_improved): 0 for an isolated vertex."""
        _, _, reached, dsum = self.raw_paths(np.arange(self.n), False, False, True)
        return closeness_from(reached, dsum, self.n, wf_improved)

    def paths(self, sources=None, normalized=True, wf_improved=True):
        """Betweenness, load and closeness from ONE shortest-path pass: {'betweenness', 'load', 'closeness'}.
        sources=None: every vertex, exactly networkx's three measures.  With a source list (e.g. sample_sources):
        betweenness and load are the sums over those sources scaled by n / len(sources) (networkx's sampled
        betweenness), and closeness holds the closeness of the listed sources, in list order."""
        if sources is None:
            src, k = np.arange(self.n, dtype=np.int64), None
        else:
            src = self._ids(sources)
            k = len(src)
        bc, ld, reached, dsum = self.raw_paths(src, True, True, True)
        scale = betweenness_scale(self.n, normalized, k)
        if scale is not None:
            bc = bc * scale
        if normalized and self.n > 2:
            ld = ld * (1.0 / ((self.n - 1) * (self.n - 2)))
        if k is not None and k > 0:
            ld = ld * (self.n / k)
        return {"betweenness": bc, "load": ld, "closeness": closeness_from(reached, dsum, self.n, wf_improved)}

    def component_labels(self):
        """(n,) int32: the smallest vertex id in every vertex's connected component (gh_cent_components)."""
        if self._g is None:
            return np.zeros(0, dtype=np.int32)
        return self._g.components()[0]

    def distances(self, sources=None):
        """Breadth-first levels from vertex ids `sources` (None: every vertex; gh_cent_distances): (reached (S,) int64,
        dist_sum (S,) int64, eccentricity (S,) int32).  reached counts the source itself; for a source that does not
        reach every vertex, eccentricity is its greatest finite distance."""
        src = np.arange(self.n, dtype=np.int64) if sources is None else np.asarray(sources, dtype=np.int64).ravel()
        if len(src) and (src.min() < 0 or src.max() >= self.n):
            raise ValueError(f"source ids must lie in [0, {self.n})")
        if self._g is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
        return self._g.distances(src)

    def triangle_counts(self):
        """(n,) int64: the number of triangles through every vertex (gh_cent_triangles)."""
        if self._g is None:
            return np.zeros(0, dtype=np.int64)
        return self._g.triangles()

    def core_layers(self):
        """(core (n,) int32, layer (n,) int32): networkx's core_number and onion_layers in vertex order, from one
        synchronous peel (gh_cent_cores)."""
        if self._g is None:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        return self._g.cores()[:2]

    def truss_numbers(self):
        """(n_edges,) int32 aligned with self.edges: the largest k whose k-truss holds the edge (gh_cent_truss)."""
        if self._g is None:
            return np.zeros(0, dtype=np.int32)
        return self._g.truss()[0]

    def link_scores(self, pairs):
        """(cn, aa, ra), (P,) int64 each, of the vertex-id pairs `pairs` ((P, 2)): common neighbours and the fixed-point
        Adamic-Adar and resource-allocation sums of include/graphem_hip.h "link scores" (gh_cent_link_scores)."""
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        if self._g is None:
            if len(pairs):
                raise ValueError("vertex ids must lie in [0, 0)")
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
        return self._g.link_scores(pairs)

    def link_candidates(self, kind, k, rows=None):
        """(ids (R, k) int32, num (R, k) int64, den (R, k) int64): the k best vertices at hop distance two of every source
        in `rows` (vertex ids; None: every vertex) under score kind `kind`, best first; unused slots hold -1, 0, 1
        (gh_cent_link_candidates)."""
        rows = np.arange(self.n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
        if self._g is None:
            if len(rows):
                raise ValueError("vertex ids must lie in [0, 0)")
            k = int(k)
            return np.zeros((0, k), np.int32), np.zeros((0, k), np.int64), np.zeros((0, k), np.int64)
        return self._g.link_candidates(kind, k, rows)

    def label_propagation(self, seed_labels, n_classes, max_rounds=100):
        """(labels (n,) int32, rounds, converged): synchronous label propagation with clamped seeds, the rule of
        include/graphem_hip.h "label propagation" (gh_cent_label_propagation).  seed_labels: (n,) ints, -1 = unlabelled,
        else a class in [0, n_classes)."""
        seed_labels = np.asarray(seed_labels).ravel()
        if len(seed_labels) != self.n:
            raise ValueError(f"{len(seed_labels)} seed labels for {self.n} vertices")
        if not 1 <= int(n_classes) <= _native.LABEL_MAX_CLASSES:
            raise ValueError(f"n_classes must lie in [1, {_native.LABEL_MAX_CLASSES}], got {n_classes}")
        if int(max_rounds) < 0:
            raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
        if self._g is None:
            return np.zeros(0, dtype=np.int32), 0, int(max_rounds) > 0
        return self._g.label_propagation(seed_labels, n_classes, max_rounds)

    def louvain_levels(self, seed=0, max_levels=32, max_rounds=1000):
        """The Louvain levels of include/graphem_hip.h "communities" (gh_cent_louvain): (labels (L, n) int32, numerators
        [L] of Python ints, n_communities (L,) int64, rounds (L,) int32, M).  labels[l][v] = the smallest vertex id in v's
        community after level l; L >= 1 for a graph with vertices (the singletons when nothing merges).  Modularity of
        level l is numerators[l] / M**2."""
        if int(max_levels) < 1 or int(max_rounds) < 1:
            raise ValueError("max_levels and max_rounds must be >= 1")
        if self._g is None:
            return np.zeros((0, 0), np.int32), [], np.zeros(0, np.int64), np.zeros(0, np.int32), 0
        return self._g.louvain(seed, max_levels, max_rounds)

    def modularity_terms(self, labels):
        """(sum I, sum T^2, M) of the labelling `labels` ((n,) ints in [0, n)), three exact Python ints
        (gh_cent_modularity): modularity = (M sum I - sum T^2) / M**2."""
        labels = np.asarray(labels).ravel()
        if len(labels) != self.n:
            raise ValueError(f"labels must have {self.n} entries")
        if self.n and (labels.min() < 0 or labels.max() >= self.n):
            raise ValueError(f"labels must lie in [0, {self.n})")
        if self._g is None:
            return 0, 0, 0
        return self._g.modularity(labels)

    def pagerank(self, alpha=0.85, max_iter=100, tol=1e-6, return_iterations=False):
        """networkx pagerank(G, alpha, max_iter=max_iter, tol=tol) (_pagerank_scipy): raises
        PowerIterationFailedConvergence when max_iter iterations do not converge."""
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError("alpha must lie in [0, 1]")
        if int(max_iter) < 1:
            raise ValueError("max_iter must be >= 1")
        if float(tol) < 0:
            raise ValueError("tol must be >= 0")
        if self._g is None:
            return (np.zeros(0), 0) if return_iterations else np.zeros(0)
        x, its = self._g.pagerank(alpha, max_iter, tol)
        if its < 0:
            raise _no_convergence(int(max_iter))
        return (x, its) if return_iterations else x

    def eigenvector(self, max_iter=None, tol=1e-12, shift=1.0):
        """networkx eigenvector_centrality_numpy(G): the Perron vector of the adjacency, unit 2-norm, positive sum.
        Lanczos (spectral._trlan) on A + shift I through gh_spmv_adj_shift; tol bounds the relative Ritz residual,
        max_iter the matvecs (default max(2000, 20 n) capped at 100000).  A disconnected graph raises AmbiguousSolution
        (ValueError without networkx), as networkx does."""
        import torch
        from scipy.sparse.csgraph import connected_components
        from .spectral import _trlan
        if self.n == 0:
            raise ValueError("cannot compute centrality for the null graph")
        if float(shift) <= 0:
            raise ValueError("shift must be > 0")
        adj = sp.coo_matrix((np.ones(len(self.edges)), (self.edges[:, 0], self.edges[:, 1])), shape=(self.n, self.n))
        if connected_components(adj, directed=False)[0] > 1:
            raise _ambiguous("`eigenvector_centrality_numpy` does not give consistent results for disconnected graphs")
        if self.n <= 2:   # connected with one or two vertices: the uniform vector (too small a Krylov space for _trlan)
            return np.full(self.n, 1.0 / np.sqrt(self.n))
        dev = torch.device(f"cuda:{self.device_id}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        g = self._g

        def apply_b(x, y):
            g.spmv_shift(stream, x.data_ptr(), y.data_ptr(), shift)

        steps = int(max_iter) if max_iter is not None else int(min(max(2000, 20 * self.n), 100000))
        gen = torch.Generator(device="cpu").manual_seed(0)
        _, X, _, _, converged = _trlan(apply_b, self.n, 1, dev, None, float(tol), steps, 10, gen)
        if not converged:
            raise _no_convergence(steps)
        v = X[:, 0].cpu().numpy().astype(np.float64)
        norm = np.sign(v.sum()) * np.linalg.norm(v)
        return v / norm

    def close(self):
        if self._g is not None:
            self._g.close()
            self._g = None


def _graph(G):
    return (G, False) if isinstance(G, CentralityGraph) else (CentralityGraph(G), True)


def _check_unweighted(G, weight):
    if weight is None or not hasattr(G, "edges"):
        return
    if any(weight in d for _, _, d in G.edges(data=True)):
        raise NotImplementedError("weighted graphs are not supported")


def betweenness_centrality(G, k=None, normalized=True, weight=None, endpoints=False, seed=None):
    """networkx.betweenness_centrality on the GPU: a dict keyed by node."""
    if weight is not None:
        raise NotImplementedError("weighted betweenness is not supported")
    if endpoints:
        raise NotImplementedError("endpoints=True is not supported")
    g, own = _graph(G)
    try:
        return g.as_dict(g.betweenness(normalized, k, seed))
    finally:
        if own:
            g.close()


def load_centrality(G, v=None, cutoff=None, normalized=True, weight=None):
    """networkx.load_centrality on the GPU: a dict keyed by node (the value of node v when v is given)."""
    if cutoff is not None:
        raise NotImplementedError("cutoff is not supported")
    if weight is not None:
        raise NotImplementedError("weighted load is not supported")
    g, own = _graph(G)
    try:
        out = g.as_dict(g.load(normalized))
    finally:
        if own:
            g.close()
    return out[v] if v is not None else out


def closeness_centrality(G, u=None, distance=None, wf_improved=True):
    """networkx.closeness_centrality on the GPU: a dict keyed by node (the value of node u when u is given)."""
    if distance is not None:
        raise NotImplementedError("weighted distances are not supported")
    g, own = _graph(G)
    try:
        if u is not None:
            _, _, reached, dsum = g.raw_paths(g._ids([u]), False, False, True)   # pylint: disable=protected-access
            return float(closeness_from(reached, dsum, g.n, wf_improved)[0])
        return g.as_dict(g.closeness(wf_improved))
    finally:
        if own:
            g.close()


def pagerank(G, alpha=0.85, personalization=None, max_iter=100, tol=1e-06, nstart=None, weight="weight", dangling=None):
    """networkx.pagerank on the GPU (uniform personalisation, unweighted): a dict keyed by node."""
    if personalization is not None or nstart is not None or dangling is not None:
        raise NotImplementedError("personalization, nstart and dangling are not supported")
    _check_unweighted(G, weight)
    g, own = _graph(G)
    try:
        if g.n == 0:
            return {}
        return g.as_dict(g.pagerank(alpha, max_iter, tol))
    finally:
        if own:
            g.close()


def eigenvector_centrality_numpy(G, weight=None, max_iter=50, tol=0):
    """networkx.eigenvector_centrality_numpy on the GPU: a dict keyed by node.  max_iter and tol are ARPACK's in
    networkx; here the Lanczos solve runs to a relative residual of 1e-12 (tol > 0: that instead)."""
    del max_iter
    _check_unweighted(G, weight)
    g, own = _graph(G)
    try:
        return g.as_dict(g.eigenvector(tol=float(tol) if tol else 1e-12))
    finally:
        if own:
            g.close()


# what the reference catches around eigenvector_centrality_numpy (benchmark.py:80-88)
_EIG_FAILURES = (ValueError,) if _nx is None else (ValueError, _nx.NetworkXError, _nx.AmbiguousSolution)


# ---- the reference's benchmark functions (benchmark.py:18-243) -------------------------------------------------------
def _generate(graph_generator, graph_params):
    out = graph_generator(**graph_params)
    if sp.issparse(out):
        adjacency = sp.csr_matrix(out)
        n = adjacency.shape[0]
        edges = np.column_stack(sp.triu(adjacency, k=1).nonzero()).astype(np.int64)
    else:
        edges = np.asarray(out, dtype=np.int64).reshape(-1, 2)
        n = max(int(edges.max()) + 1 if len(edges) else 0, int(graph_params.get("n", 0)))
        adjacency = None
    return n, edges, adjacency


def run_benchmark(graph_generator, graph_params, dim=3, L_min=10.0, k_attr=0.5, k_inter=0.1, n_neighbors=15,
                  sample_size=512, num_iterations=40, backend="hip", *, betweenness_k=None, cores=False, **kwargs):
    """The reference's run_benchmark (benchmark.py:18-160) with every centrality on the GPU and this package's embedder:
    the reference's result keys, plus 'centrality_time' (seconds spent on the six centralities) and 'betweenness_k'.
    The generator may return an (E, 2) edge array or an adjacency matrix.

    betweenness_k: None -- exact betweenness and load (every vertex a source, as the reference); an int -- both from
    networkx's sample of that many sources (random.Random(seed).sample over the nodes, seed = kwargs' 'seed' or 0),
    scaled by n / k.  Closeness stays exact: it comes from the same pass when betweenness_k is None, else from a
    distances-only pass over every vertex.  A disconnected graph has no eigenvector centrality; as in the reference, degree
    centrality stands in for it.

    cores=True adds 'core_number' and 'onion_layer' (float arrays; CentralityGraph.core_layers), counted in
    'centrality_time'."""
    from . import create_graphem, edges_to_adjacency
    start_time = time.time()
    n, edges, adjacency = _generate(graph_generator, graph_params)
    m = len(edges)
    if adjacency is None:
        adjacency = edges_to_adjacency(n, edges)

    c0 = time.time()
    g = CentralityGraph(edges, n=n)
    degree = g.degree()
    if betweenness_k is None:
        paths = g.paths()
    else:
        src = sample_sources(range(n), int(betweenness_k), int(kwargs.get("seed") or 0))
        paths = g.paths(src)
        paths["closeness"] = g.closeness()
    try:
        eigenvector = g.eigenvector()
    except _EIG_FAILURES as e:
        logger.warning("Eigenvector centrality calculation failed: %s; using degree centrality", e)
        eigenvector = degree / (n - 1.0) if n > 1 else np.ones(n)
    pr = g.pagerank()
    core_layers = g.core_layers() if cores else None
    g.close()
    centrality_time = time.time() - c0

    embedder = create_graphem(adjacency, n_components=dim, backend=backend, L_min=L_min, k_attr=k_attr, k_inter=k_inter,
                              n_neighbors=n_neighbors, sample_size=sample_size, verbose=False, **kwargs)
    layout_start = time.time()
    embedder.run_layout(num_iterations=num_iterations)
    layout_time = time.time() - layout_start
    positions = np.array(embedder.positions)
    radii = np.linalg.norm(positions, axis=1)

    result = {
        "n": n,
        "m": m,
        "density": 2 * m / (n * (n - 1)) if n > 1 else 0.0,
        "avg_degree": 2 * m / n if n > 0 else 0.0,
        "layout_time": layout_time,
        "graph_type": graph_generator.__name__,
        "n_components": dim,
        "backend": backend,
        "radii": radii,
        "positions": positions,
        "degree": degree,
        "betweenness": paths["betweenness"],
        "eigenvector": eigenvector,
        "pagerank": pr,
        "closeness": paths["closeness"],
        "node_load": paths["load"],
        "centrality_time": centrality_time,
        "betweenness_k": betweenness_k,
    }
    if cores:
        result["core_number"] = core_layers[0].astype(np.float64)
        result["onion_layer"] = core_layers[1].astype(np.float64)
    result["total_time"] = time.time() - start_time
    return result


CORRELATION_KEYS = ("degree", "betweenness", "eigenvector", "pagerank", "closeness", "node_load")
CORE_KEYS = ("core_number", "onion_layer")


def benchmark_correlations(graph_generator, graph_params, dim=2, L_min=10.0, k_attr=0.5, k_inter=0.1, n_neighbors=15,
                           sample_size=512, num_iterations=40, backend="hip", *, betweenness_k=None, bootstrap_reps=None,
                           bootstrap_seed=0, cores=False, **kwargs):
    """The reference's benchmark_correlations (benchmark.py:163-243): run_benchmark, then Spearman's rho (and p) between
    the radii and each centrality under results['correlations'][name] = {'rho', 'p'}.

    bootstrap_reps: None -- exactly that; an int -- every entry also gets 'ci_low' and 'ci_high', the 2.5 and 97.5
    percentiles of that many bootstrap replicates (visualization.bootstrap_spearman with seed bootstrap_seed).
    cores=True: run_benchmark's 'core_number' and 'onion_layer' arrays, correlated like the six centralities."""
    from scipy import stats
    results = run_benchmark(graph_generator, graph_params, dim=dim, L_min=L_min, k_attr=k_attr, k_inter=k_inter,
                            n_neighbors=n_neighbors, sample_size=sample_size, num_iterations=num_iterations,
                            backend=backend, betweenness_k=betweenness_k, cores=cores, **kwargs)
    names = CORRELATION_KEYS + (CORE_KEYS if cores else ())
    radii = results["radii"]
    correlations = {}
    for name in names:
        rho, p = stats.spearmanr(radii, results[name])
        correlations[name] = {"rho": rho, "p": p}
    if bootstrap_reps is not None:
        from .visualization import bootstrap_spearman
        _, _, ci_low, ci_high, _ = bootstrap_spearman(radii, [results[name] for name in names],
                                                      reps=bootstrap_reps, seed=bootstrap_seed)
        for j, name in enumerate(names):
            correlations[name]["ci_low"] = float(ci_low[j])
            correlations[name]["ci_high"] = float(ci_high[j])
    results["correlations"] = correlations
    return results
