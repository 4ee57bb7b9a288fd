"""Influence estimation and greedy seed selection: Monte Carlo Independent Cascade on the GPU.

The reference (graphem_rapids/influence.py, benchmark.py:246-379) scores seed sets with one pure-Python ndlib cascade and
selects greedy seeds with k * n of them.  Here every cascade runs in csrc/influence.hip (gh_ic_spread), thousands of
trials per call, with counter-based coins (include/graphem_hip.h): a result depends only on the arc set, the seed set,
p, max_hops, the number of trials and the seed, and tests/ic_reference.py recomputes it bit for bit in numpy.

Reverse influence sampling (RIS) draws reverse-reachable sets with the same coins (gh_ic_rr_sample) and selects seeds by
greedy maximum coverage on the device (gh_rr_cover): a baseline whose cost follows the sizes of the sets, not
n * trials * k, for the graph sizes CELF cannot reach (tests/ris_reference.py restates the rule in numpy).

Per-arc probabilities.  Wherever p is accepted it may be, instead of one float for the whole graph, a specification that
arc_probabilities resolves to one probability per directed arc: "wc" (weighted cascade, p(u -> v) = 1 / indeg(v)), an
array aligned with InfluenceGraph.arcs, or a sparse matrix P[u, v].  The coin of an arc and its key do not change; only
the threshold it is compared with becomes the arc's own (include/graphem_hip.h), so the two directions of an undirected
edge share a coin but may differ in probability.  A float takes gh_ic_spread / gh_ic_rr_sample as before; a table is
uploaded once per distinct specification (gh_ic_set_arc_probabilities) and read by gh_ic_spread_arcs /
gh_ic_rr_sample_arcs, and tests/arc_ic_reference.py recomputes every result bit for bit.

Linear Threshold.  p may also be linear_threshold(w): the other canonical diffusion model (Kempe, Kleinberg, Tardos 2003),
in its live-edge form -- in a trial every vertex selects at most one in-arc, arc u -> v with probability w_uv, by one
32-bit pick per (trial, vertex) against fixed-point intervals of the vertex's in-arcs (include/graphem_hip.h).  lt_weights
resolves w to one weight per directed arc; the table is uploaded once per distinct specification (gh_ic_set_lt_weights)
beside the per-arc table, gh_ic_spread_lt / gh_ic_rr_sample_lt read it, and tests/lt_reference.py recomputes every result
bit for bit.  max_hops counts rounds of the threshold process.
"""
import hashlib
import heapq
import math
import numbers
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


def _checked_probabilities(prob):
    if prob.size and not (np.all(prob >= 0.0) and np.all(prob <= 1.0)):   # a NaN fails both comparisons
        raise ValueError("arc probabilities must lie in [0, 1] and must not be NaN")
    return prob


def arc_probabilities(arcs, n, directed, p):
    """One probability per directed arc from the specification p, against the canonical (A, 2) arc array of _graph_arcs
    (unique rows in ascending order, no self-loops, an undirected edge as (a, b) with a < b).  Host only.

    Returns float64 (A,) for a directed graph, (A, 2) for an undirected one: column 0 is a -> b, column 1 is b -> a.
    p: "wc" / "weighted_cascade" -- p(u -> v) = 1 / indeg(v), for an undirected graph 1 / deg(v);
       an (A,) array aligned with arcs (both directions of an undirected edge get the value);
       an (A, 2) array, undirected graphs only: the a -> b and b -> a probabilities;
       a scipy sparse (n, n) matrix, P[u, v] = p(u -> v): an absent entry is 0, a stored entry on a pair that is not an
       arc raises.
    ValueError for anything else: a float (that is the uniform model, which needs no table), a wrong shape, NaN, values
    outside [0, 1]."""
    arcs = np.asarray(arcs, dtype=np.int64).reshape(-1, 2)
    n, directed, A = int(n), bool(directed), len(arcs)
    a, b = arcs[:, 0], arcs[:, 1]
    if isinstance(p, str):
        if p not in ("wc", "weighted_cascade"):
            raise ValueError(f"unknown probability model {p!r}: 'wc' / 'weighted_cascade' is the one with a name")
        if directed:
            return 1.0 / np.bincount(b, minlength=n)[b].astype(np.float64)
        deg = np.bincount(arcs.ravel(), minlength=n).astype(np.float64)
        return np.column_stack([1.0 / deg[b], 1.0 / deg[a]])
    if sp.issparse(p):
        if p.shape != (n, n):
            raise ValueError(f"a probability matrix must have shape ({n}, {n}), got {p.shape}")
        coo = sp.coo_matrix(p)
        coo.sum_duplicates()
        u, v, val = coo.row.astype(np.int64), coo.col.astype(np.int64), _checked_probabilities(coo.data.astype(np.float64))
        lo, hi = (u, v) if directed else (np.minimum(u, v), np.maximum(u, v))
        slot = np.searchsorted(a * n + b, lo * n + hi)   # the canonical rows ascend, so their keys do
        hit = slot < A
        hit[hit] = (a[slot[hit]] == lo[hit]) & (b[slot[hit]] == hi[hit])
        if not hit.all():
            i = int(np.flatnonzero(~hit)[0])
            raise ValueError(f"the probability matrix stores an entry at ({u[i]}, {v[i]}), which is not an arc of the graph")
        out = np.zeros(A if directed else (A, 2), dtype=np.float64)
        if directed:
            out[slot] = val
        else:
            out[slot, (u > v).astype(np.int64)] = val
        return out
    if isinstance(p, numbers.Number) or p is None:
        raise ValueError("a per-arc specification is 'wc', an array aligned with the arcs or a sparse matrix")
    try:
        prob = np.array(p, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"not a per-arc probability specification: {exc}") from None
    if prob.shape == (A,):
        _checked_probabilities(prob)
        return prob if directed else np.column_stack([prob, prob])
    if prob.shape == (A, 2) and not directed:
        return _checked_probabilities(prob)
    want = f"({A},)" if directed else f"({A},) or ({A}, 2)"
    raise ValueError(f"a probability array must have shape {want}, got {prob.shape}")


def trivalency_probabilities(arcs, directed, seed=0, values=(0.1, 0.01, 0.001)):
    """The trivalency model: every directed arc draws its probability from `values`,
    np.random.default_rng(seed).choice(values, size=...), in arc_probabilities' shape for the canonical arc array."""
    A = len(np.asarray(arcs).reshape(-1, 2))
    return np.random.default_rng(seed).choice(np.asarray(values, dtype=np.float64), size=A if directed else (A, 2))


_LT_ROW_MARGIN = 1.0 + 2.0 ** -20   # include/graphem_hip.h: what the sequential double sum of a row may reach


def _lt_rows(arcs, directed, weight):
    """(src, dst, w) of every directed arc of canonical arcs and lt_weights' array, by (target, source) ascending: the
    order in which the header sums a row."""
    a, b = arcs[:, 0], arcs[:, 1]
    if directed:
        src, dst, w = a, b, weight
    else:
        src, dst, w = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([weight[:, 0], weight[:, 1]])
    order = np.lexsort((src, dst))
    return src[order], dst[order], w[order]


def lt_weights(arcs, n, directed, w="uniform"):
    """One Linear Threshold weight per directed arc from the specification w, against the canonical (A, 2) arc array of
    _graph_arcs.  Host only.  Returns arc_probabilities' shapes: float64 (A,) for a directed graph, (A, 2) -- a -> b,
    b -> a -- for an undirected one, whose two arcs of an edge are weighted separately.
    w: "uniform" -- w_uv = 1 / indeg(v), for an undirected graph 1 / deg(v): ndlib's ThresholdModel, which compares the
       fraction of active neighbours with the threshold;
       an (A,) array aligned with arcs (both arcs of an undirected edge get the value), or an (A, 2) array;
       a scipy sparse (n, n) matrix, W[u, v] = w_uv: an absent entry is 0.
    ValueError for NaN, a weight outside [0, 1], a wrong shape, a stored entry on a pair that is not an arc, and a vertex
    whose in-weights, summed in ascending source id, exceed 1 + 2^-20 (the header derives the margin)."""
    arcs = np.asarray(arcs, dtype=np.int64).reshape(-1, 2)
    n, directed = int(n), bool(directed)
    if isinstance(w, str):
        if w != "uniform":
            raise ValueError(f"unknown Linear Threshold weighting {w!r}: 'uniform' is the one with a name")
        return arc_probabilities(arcs, n, directed, "wc")
    try:
        weight = arc_probabilities(arcs, n, directed, w)
    except ValueError as exc:
        raise ValueError(f"Linear Threshold weights: {exc}") from None
    _, dst, ws = _lt_rows(arcs, directed, weight)
    total = np.bincount(dst, weights=ws, minlength=n)   # adds in array order: the sequential sum of every row
    if len(total) and total.max() > _LT_ROW_MARGIN:
        v = int(np.argmax(total > _LT_ROW_MARGIN))
        raise ValueError(f"the Linear Threshold weights into vertex {v} sum to {total[v]!r}, above 1 + 2^-20")
    return weight


class LinearThreshold:
    """What linear_threshold returns: a diffusion-model specification that every p parameter accepts."""

    def __init__(self, w="uniform"):
        self.w = w

    def __repr__(self):
        return f"linear_threshold({self.w!r})" if isinstance(self.w, str) else "linear_threshold(<weights>)"


def linear_threshold(w="uniform"):
    """The Linear Threshold model as a value for p: InfluenceGraph.spread / marginal_totals / greedy / rr_sets,
    RRCollection.extend, influence_spread, ndlib_estimated_influence, greedy_seed_selection, ris_seed_selection and
    run_influence_benchmark take it wherever they take a probability.  w: what lt_weights takes.  The specification is
    resolved against the graph when a call first meets it, and its table is uploaded once (a digest of the resolved
    weights tells).  Hops keep the package's iterations_count - 2 convention, which is the package's own here: ndlib's
    threshold model has no "removed" state, so nothing in ndlib lags the active set by two iterations."""
    return LinearThreshold(w)


class _LTTable:
    """A resolved Linear Threshold specification: the host weights and their digest, as _ArcTable is for probabilities."""

    def __init__(self, weight):
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)
        self.weight.setflags(write=False)
        self.key = hashlib.blake2b(self.weight.tobytes(), digest_size=16).digest()


class _ArcTable:
    """A resolved specification: its own copy of the host array, and the digest an InfluenceGraph compares with the
    table its handle holds, so one specification is uploaded once however many calls name it."""

    def __init__(self, prob):
        self.prob = np.ascontiguousarray(prob, dtype=np.float64)
        self.prob.setflags(write=False)
        self.key = hashlib.blake2b(self.prob.tobytes(), digest_size=16).digest()


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
    order; seeds are given and returned as labels.

    p, wherever a method takes it, is one float for the whole graph, linear_threshold(w) for the Linear Threshold model,
    or a per-arc specification (arc_probabilities): "wc", an array aligned with self.arcs, a sparse matrix.  The handle keeps the table of the last specification used, so
    repeated calls with one specification upload it once; a float never touches it."""

    def __init__(self, graph, n=None, directed=None, device_id=0):
        self.n, self.arcs, self.directed, self.labels = _graph_arcs(graph, n, directed)
        self._index = None if self.labels is None else {v: i for i, v in enumerate(self.labels)}
        self._device_id = int(device_id)
        self._ic = _native.ICGraph(max(self.n, 1), self.arcs, self.directed, device_id) if self.n > 0 else None
        self._table_key = None   # digest of the table the handle holds
        self._lt_key = None      # and of its Linear Threshold table

    def arc_probabilities(self, p):
        """The host array a per-arc specification resolves to on this graph (arc_probabilities): float64 (A,) aligned
        with self.arcs for a directed graph, (A, 2) -- a -> b, b -> a -- for an undirected one."""
        return np.array(self._resolve_table(p).prob)

    def lt_weights(self, w="uniform"):
        """The host array a Linear Threshold specification resolves to on this graph (lt_weights)."""
        return lt_weights(self.arcs, self.n, self.directed, w.w if isinstance(w, LinearThreshold) else w)

    def _resolve_table(self, p):
        return p if isinstance(p, _ArcTable) else _ArcTable(arc_probabilities(self.arcs, self.n, self.directed, p))

    def _resolve(self, p):
        """A float stays a float (the uniform path); anything else becomes an _ArcTable, resolved once per public call."""
        if isinstance(p, numbers.Real) and not isinstance(p, bool):
            return float(p)
        if isinstance(p, _LTTable):
            return p
        if isinstance(p, LinearThreshold):
            return _LTTable(lt_weights(self.arcs, self.n, self.directed, p.w))
        return self._resolve_table(p)

    def _native_p(self, p):
        """What _native.ICGraph takes for a resolved p: the float, or None / _native.LT once the handle holds p's table."""
        if isinstance(p, _LTTable):
            if self._lt_key != p.key:
                if self.directed:
                    pairs, weight = self.arcs, p.weight
                else:
                    pairs = np.concatenate([self.arcs, self.arcs[:, ::-1]])
                    weight = np.concatenate([p.weight[:, 0], p.weight[:, 1]])
                self._ic.set_lt_weights(pairs, weight)
                self._lt_key = p.key
            return _native.LT
        if not isinstance(p, _ArcTable):
            return p
        if self._table_key != p.key:
            if self.directed:
                pairs, prob = self.arcs, p.prob
            else:
                pairs, prob = np.concatenate([self.arcs, self.arcs[:, ::-1]]), np.concatenate([p.prob[:, 0], p.prob[:, 1]])
            self._ic.set_arc_probabilities(pairs, prob)
            self._table_key = p.key
        return None

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
        p = self._resolve(p)
        if self._ic is None:
            trials = np.zeros(int(n_trials), dtype=np.int32)
        else:
            _, trials = self._ic.spread([ids], self._native_p(p), n_trials, seed, self._hops(max_hops), per_trial=True)
            trials = trials[0]
        mean = float(trials.sum(dtype=np.int64)) / int(n_trials)
        return (mean, trials) if return_trials else mean

    def marginal_totals(self, base, candidates, p, n_trials, max_hops=None, seed=0):
        """(len(candidates),) int64: sum over trials of |R(base + c)| - |R(base)|, the same coins for every candidate."""
        cand = np.asarray(candidates, dtype=np.int64).ravel()
        p = self._resolve(p)
        if self._ic is None or len(cand) == 0:
            return np.zeros(len(cand), dtype=np.int64)
        return self._ic.spread(cand.reshape(-1, 1), self._native_p(p), n_trials, seed, self._hops(max_hops),
                               base=np.asarray(base, dtype=np.int64))

    def greedy(self, k, p=0.1, n_trials=256, max_hops=None, seed=0, celf=True):
        """Greedy seeds maximising the sample-average spread over ONE fixed set of n_trials coin draws (common random
        numbers): (seeds, candidate evaluations)."""
        p = self._resolve(p)   # once: every evaluation then finds the handle's table in place

        def evaluate(base, cand):
            return self.marginal_totals(base, cand, p, n_trials, max_hops, seed)
        seeds, evals = celf_greedy(evaluate, self.n, k, celf=celf)
        if self.labels is not None:
            seeds = [self.labels[s] for s in seeds]
        return seeds, evals

    def rr_sets(self, n_samples, p=0.1, max_hops=None, seed=0, trials=None, roots=None):
        """An RRCollection of n_samples reverse-reachable sets: sample j is the search backwards from roots[j] over the
        live arcs of trial trials[j] (defaults: trial j, the root the header derives from the trial's word).  roots are
        given as labels where the graph has labels."""
        if self._ic is None:
            raise ValueError("the graph has no vertices")
        p = self._resolve(p)
        coll = RRCollection(_native.RRSets(self.n, self._device_id), self, p, self._hops(max_hops), seed)
        try:
            coll.extend(n_samples, trials, roots)
        except Exception:
            coll.close()
            raise
        return coll

    def close(self):
        if self._ic is not None:
            self._ic.close()


class RRCollection:
    """Reverse-reachable sets on the device (gh_rr_*): InfluenceGraph.rr_sets draws them, max_coverage uploads any set
    system.  indptr (int64), members (int32 vertex ids, ascending within a set) and roots (int32 ids) are downloaded on
    first use; cover and count_hit speak the graph's labels."""

    def __init__(self, rr, graph=None, p=None, hops=-1, seed=0):
        self._rr, self._graph, self._p, self._hops, self._seed = rr, graph, p, hops, seed
        self._host = None

    @property
    def n_sets(self):
        return self._rr.counts()[0]

    @property
    def n_members(self):
        return self._rr.counts()[1]

    def __len__(self):
        return self.n_sets

    def _download(self):
        if self._host is None:
            self._host = self._rr.download()
        return self._host

    indptr = property(lambda self: self._download()[0])
    members = property(lambda self: self._download()[1])
    roots = property(lambda self: self._download()[2])

    def set_memory_budget(self, nbytes):
        """Device bytes the collection may hold (0: the default, 4 GiB); a draw that would outgrow it raises MemoryError."""
        self._rr.set_memory_budget(nbytes)

    def extend(self, n_samples, trials=None, roots=None):
        """Appends n_samples sets drawn with the collection's p, max_hops and seed; default trials continue at n_sets."""
        if self._graph is None:
            raise ValueError("an uploaded set system has no graph to sample from")
        if roots is not None:
            roots = self._graph._ids(roots)
        self._host = None
        self._graph._ic.rr_sample(self._rr, n_samples, self._graph._native_p(self._p), self._seed, self._hops, trials, roots)
        return self

    def _labels(self):
        return None if self._graph is None else self._graph.labels

    def cover(self, k):
        """Greedy maximum coverage: (seeds, gains) of min(k, n) rounds; gains int64, the newly covered sets per round."""
        seeds, gains = self._rr.cover(k)
        labels = self._labels()
        seeds = [int(v) for v in seeds] if labels is None else [labels[v] for v in seeds]
        return seeds, gains

    def count_hit(self, vertices):
        """Sets that contain at least one of the vertices."""
        ids = self._graph._ids(vertices) if self._graph is not None else np.asarray(list(vertices), dtype=np.int64)
        return self._rr.count_hit(ids)

    def close(self):
        self._rr.close()


def max_coverage(indptr, members, n, k, device_id=0):
    """Greedy maximum coverage of the set system (indptr, members) over the vertices 0 .. n-1 on the GPU: set s holds
    members[indptr[s]:indptr[s + 1]], ascending.  Each of min(k, n) rounds takes the unchosen vertex in the most uncovered
    sets, ties to the smallest id.  Returns (seeds, gains)."""
    coll = RRCollection(_native.RRSets(int(n), device_id))
    try:
        coll._rr.upload(indptr, members)
        return coll.cover(k)
    finally:
        coll.close()


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


_E1 = 1.0 - 1.0 / math.e


def opim_sample_plan(n, k, epsilon, delta, max_samples=None):
    """(theta_0, theta_max, i_max, a) of the OPIM-C stopping rule (Tang, Tang, Xiao, Yuan 2018)."""
    ln6d = math.log(6.0 / delta)
    ln_binom = math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)
    theta_max = math.ceil(2.0 * n * (_E1 * math.sqrt(ln6d) + math.sqrt(_E1 * (ln_binom + ln6d))) ** 2 / (epsilon ** 2 * k))
    if max_samples is not None:
        theta_max = min(theta_max, int(max_samples))
    theta_max = max(1, theta_max)
    theta_0 = max(1, math.ceil(theta_max * epsilon ** 2 * k / n))
    i_max = max(1, math.ceil(math.log2(theta_max / theta_0)))
    return theta_0, theta_max, i_max, math.log(3.0 * i_max / delta)


def opim_bounds(gain_sum, hit2, theta, n, a):
    """(lower bound of the spread of S, upper bound of the optimum) from Lambda1 = sets of R1 the greedy seeds cover and
    Lambda2 = sets of R2 they hit, theta sets each."""
    inner = math.sqrt(hit2 + 2.0 * a / 9.0) - math.sqrt(a / 2.0)
    lower = 0.0 if inner < 0 else max(0.0, inner * inner - a / 18.0) * n / theta
    upper = (math.sqrt(gain_sum / _E1 + a / 2.0) + math.sqrt(a / 2.0)) ** 2 * n / theta
    return lower, upper


def opim_c(sample, cover, count, n, k, epsilon, delta=None, max_samples=None):
    """The OPIM-C driver over three callables, as celf_greedy is written over an evaluator:
    sample(theta) grows both collections to theta sets each -- R1 on trials 0, 2, 4, .., R2 on trials 1, 3, 5, .., so a
    doubling extends prefixes; cover(k) -> (seeds, gains) by greedy maximum coverage of R1; count(seeds) -> sets of R2 hit.
    Stops when lower / upper >= 1 - 1/e - epsilon or after i_max doublings.  Returns (seeds, info)."""
    k = min(int(k), n)
    delta = 1.0 / n if delta is None else float(delta)
    if not 0 < epsilon < 1 or not 0 < delta < 1:
        raise ValueError("epsilon and delta must lie in (0, 1)")
    if k <= 0:
        return [], {"samples": 0, "covered": 0, "estimated_influence": 0.0, "rounds": 0, "lower": 0.0, "upper": 0.0, "ratio": 0.0}
    theta, theta_max, i_max, a = opim_sample_plan(n, k, epsilon, delta, max_samples)
    for i in range(1, i_max + 1):
        sample(theta)
        seeds, gains = cover(k)
        covered = int(np.sum(gains))
        lower, upper = opim_bounds(covered, int(count(seeds)), theta, n, a)
        ratio = lower / upper
        if ratio >= _E1 - epsilon or i == i_max:
            break
        theta *= 2
    return list(seeds), {"samples": theta, "covered": covered, "estimated_influence": n * covered / theta, "rounds": i,
                         "lower": lower, "upper": upper, "ratio": ratio}


def ris_seed_selection(G, k, p=0.1, iterations_count=200, *, n_samples=None, epsilon=None, delta=None, max_samples=None,
                       seed=None):
    """Seeds by reverse influence sampling: (seeds, info), with greedy_seed_selection's conventions (hops =
    iterations_count - 2, seed=None drawn from numpy's generator, G may be an InfluenceGraph).

    n_samples = theta: one collection on trials 0 .. theta-1, then greedy maximum coverage.  epsilon (delta = 1/n by
    default; epsilon = 0.1 when neither mode is named): OPIM-C, doubling two collections until the seeds are within
    1 - 1/e - epsilon of the optimum with probability 1 - delta, at most max_samples sets each.
    info: samples, covered, estimated_influence = n * covered / samples, rounds, and lower, upper, ratio with epsilon."""
    if n_samples is not None and epsilon is not None:
        raise ValueError("give n_samples (fixed mode) or epsilon (OPIM-C), not both")
    if n_samples is None and epsilon is None:
        epsilon = 0.1
    if n_samples is not None and int(n_samples) < 1:
        raise ValueError("n_samples must be >= 1")
    if int(k) < 0:
        raise ValueError("k must be >= 0")
    seed = _draw_seed(seed)
    g = G if isinstance(G, InfluenceGraph) else InfluenceGraph(G)
    p = g._resolve(p)   # once: both collections and every doubling then find the handle's table in place
    hops = _ndlib_hops(int(iterations_count))
    k = min(int(k), g.n)
    if hops is None or k == 0:   # nothing is ever removed: every gain is 0, the choice is 0, 1, 2, ...
        seeds = list(range(k)) if g.labels is None else [g.labels[s] for s in range(k)]
        info = {"samples": 0, "covered": 0, "estimated_influence": 0.0, "rounds": 0}
        if epsilon is not None:
            info.update(lower=0.0, upper=0.0, ratio=0.0)
        return seeds, info
    if n_samples is not None:
        coll = g.rr_sets(int(n_samples), p, hops, seed)
        try:
            seeds, gains = coll.cover(k)
        finally:
            coll.close()
        covered = int(gains.sum())
        return seeds, {"samples": int(n_samples), "covered": covered, "estimated_influence": g.n * covered / int(n_samples),
                       "rounds": 1}
    r1, r2 = g.rr_sets(0, p, hops, seed), g.rr_sets(0, p, hops, seed)

    def sample(theta):
        have = len(r1)
        r1.extend(theta - have, trials=2 * np.arange(have, theta, dtype=np.uint64))
        r2.extend(theta - have, trials=2 * np.arange(have, theta, dtype=np.uint64) + np.uint64(1))
    try:
        return opim_c(sample, r1.cover, r2.count_hit, g.n, k, float(epsilon), delta, max_samples)
    finally:
        r1.close()
        r2.close()


def kshell_seed_selection(G, k):
    """The k-shell baseline for influential spreaders (Kitsak et al. 2010): the k vertices first in the order (core number
    descending, onion layer descending, degree descending, vertex id ascending), as nodes.  A pure function of the graph:
    no coins, one peel on the GPU (gh_cent_cores).  G: what CentralityGraph takes, a CentralityGraph, or an undirected
    InfluenceGraph.  ValueError for k outside [0, n]."""
    from .centrality import CentralityGraph   # centrality imports this module
    if isinstance(G, InfluenceGraph):
        if G.directed:
            raise NotImplementedError("k-shell seeds are for undirected graphs")
        g, own, labels = CentralityGraph(G.arcs, n=G.n), True, G.labels
    elif isinstance(G, CentralityGraph):
        g, own, labels = G, False, G.labels
    else:
        g, own = CentralityGraph(G), True
        labels = g.labels
    try:
        k = int(k)
        if k < 0 or k > g.n:
            raise ValueError(f"k must lie in [0, {g.n}]")
        core, layer = g.core_layers()
        order = np.lexsort((np.arange(g.n), -g.degree(), -layer.astype(np.int64), -core.astype(np.int64)))[:k]
        return order.tolist() if labels is None else [labels[i] for i in order]
    finally:
        if own:
            g.close()


def run_influence_benchmark(graph_generator, graph_params, k=10, p=0.1, iterations=200, dim=3, num_layout_iterations=20,
                            layout_params=None, backend="hip", ris=False, kshell=False):
    """The reference's run_influence_benchmark (benchmark.py:246-379) on this package's embedder and the functions above:
    GraphEm seeds against greedy seeds and a random baseline, each scored with ndlib_estimated_influence.  The generator
    may return an (E, 2) edge array or an adjacency matrix.  Returns the reference's result keys; ris=True adds
    ris_seeds, ris_influence, ris_time and ris_samples from ris_seed_selection (epsilon = 0.1); kshell=True adds
    kshell_seeds, kshell_influence and kshell_time from kshell_seed_selection.  p may be a per-arc specification
    (arc_probabilities), e.g. p="wc" for the weighted cascade, or linear_threshold() to run every selection and every
    score under the Linear Threshold model."""
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
    p = graph._resolve(p)   # a per-arc specification ("wc", ..) is resolved once for all the calls below
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
    ris_results = {}
    if ris:
        ris_start = time.time()
        ris_seeds, ris_info = ris_seed_selection(graph, k, p, iterations)
        ris_results = {"ris_seeds": ris_seeds, "ris_time": time.time() - ris_start, "ris_samples": ris_info["samples"],
                       "ris_influence": ndlib_estimated_influence(graph, ris_seeds, p, iterations)[0]}
    kshell_results = {}
    if kshell:
        kshell_start = time.time()
        kshell_seeds = kshell_seed_selection(graph, k)
        kshell_results = {"kshell_seeds": kshell_seeds, "kshell_time": time.time() - kshell_start,
                          "kshell_influence": ndlib_estimated_influence(graph, kshell_seeds, p, iterations)[0]}
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
    results.update(ris_results)
    results.update(kshell_results)
    results["total_time"] = time.time() - start_time
    return results
