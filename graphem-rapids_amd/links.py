"""Link prediction on the GPU: the classical neighbourhood predictors under networkx's names, two-hop candidate lists, and
the held-out-edge evaluation of an embedding against them.

jaccard_coefficient, adamic_adar_index, resource_allocation_index and preferential_attachment give networkx's (u, v, p)
triples; link_scores gives all of them for a list of pairs at once; link_candidates gives every source's k best vertices
at hop distance two, and top_links the k best non-adjacent pairs of the whole graph.  Two integer-exact HIP calls over
the centrality handle's CSR do the work (csrc/links.hip: gh_cent_link_scores, gh_cent_link_candidates); include/graphem_hip.h
"link scores" states the rule: common-neighbour counts, and Adamic-Adar / resource-allocation sums in fixed point of scale
2^32, so every float here is one float64 division of exact integers.

split_edges hides a share of the edges, embedding_link_scores scores pairs by an embedding (minus the squared distance),
ranking_auc and average_precision read a ranking of held-out edges against non-edges, and link_prediction_benchmark puts
them together: split, embed the train graph, score the held-out edges and as many non-edges with the embedding and with
the five predictors on the train graph.

Every graph function takes what CentralityGraph takes -- a networkx Graph, a scipy sparse adjacency (this package's graph
type), an (E, 2) edge array or a CentralityGraph.  Undirected, unweighted graphs only; self-loops are dropped and duplicate
edges merged, like the rest of the package.
"""
import functools
import time

import numpy as np
import scipy.sparse as sp

from . import _native
from .centrality import CentralityGraph, _generate, _nx
from .graphstats import _with_graph
from .influence import _graph_arcs

# ebunch=None lists every non-edge: (n choose 2) pairs on the host, 8.4 million at this size
MAX_ALL_PAIRS_VERTICES = 4096
LINK_SCORES = tuple(_native.LINK_KINDS)
LINK_METHODS = ("embedding",) + LINK_SCORES
_SCALE = 4294967296.0   # the fixed-point scale of the Adamic-Adar and resource-allocation sums
_FIXED_POINT = ("adamic_adar", "resource_allocation")


def _check_score(score):
    if score not in _native.LINK_KINDS:
        raise ValueError(f"score must be one of {LINK_SCORES}, got {score!r}")
    return score


def _node_ids(g, nodes):
    """Vertex ids of `nodes`; a node the graph does not have raises networkx's NodeNotFound (ValueError without networkx)."""
    nodes = list(nodes)
    try:
        return g._ids(nodes)   # pylint: disable=protected-access
    except (KeyError, ValueError) as e:
        missing = e.args[0] if isinstance(e, KeyError) else next(v for v in nodes if not 0 <= int(v) < g.n)
        raise (_nx.NodeNotFound if _nx is not None else ValueError)(f"Node {missing} not in G.") from None


def _pair_ids(g, pairs):
    """(P, 2) int64 vertex ids of an iterable of node pairs."""
    pairs = [tuple(p) for p in pairs]
    if any(len(p) != 2 for p in pairs):
        raise ValueError("every pair must have two nodes")
    return _node_ids(g, [x for p in pairs for x in p]).reshape(-1, 2)


def _non_edges(g):
    """Every non-adjacent vertex pair u < v, in (u, v) order."""
    if g.n > MAX_ALL_PAIRS_VERTICES:
        raise ValueError(f"ebunch=None lists every non-edge, which is limited to graphs of {MAX_ALL_PAIRS_VERTICES} vertices; "
                         f"this one has {g.n}: give an ebunch, or take the best pairs from link_candidates / top_links")
    free = np.triu(np.ones((g.n, g.n), dtype=bool), k=1)
    free[g.edges[:, 0], g.edges[:, 1]] = False
    return np.argwhere(free).astype(np.int64)


def _scores(g, ids):
    """The dict of link_scores for (P, 2) vertex ids."""
    cn, aa, ra = g.link_scores(ids)
    deg = g.degree()
    du, dv = deg[ids[:, 0]], deg[ids[:, 1]]
    uni = du + dv - cn
    return {
        "common_neighbors": cn,
        "union": uni,
        "jaccard": np.divide(cn, uni, out=np.zeros(len(ids)), where=uni > 0),
        "adamic_adar": aa / _SCALE,
        "resource_allocation": ra / _SCALE,
        "preferential_attachment": du * dv,
    }


def link_scores(G, pairs):
    """Every neighbourhood score of the node pairs `pairs` (an iterable of (u, v); u = v and adjacent pairs are allowed), in
    their order: {'common_neighbors', 'union', 'preferential_attachment'} int64 arrays and {'jaccard', 'adamic_adar',
    'resource_allocation'} float64 arrays.  jaccard is 0.0 where the union is empty, as in networkx."""
    return _with_graph(G, lambda g: _scores(g, _pair_ids(g, pairs)))


def _predict(G, ebunch, score):
    def run(g):
        if ebunch is None:
            ids = _non_edges(g)
            nodes = g.nodes
            named = [(nodes[u], nodes[v]) for u, v in ids.tolist()]
        else:
            named = [tuple(p) for p in ebunch]
            ids = _pair_ids(g, named)
        values = _scores(g, ids)[score].tolist()   # Python floats, or ints for preferential attachment
        return [(u, v, p) for (u, v), p in zip(named, values)]
    return _with_graph(G, run)


def jaccard_coefficient(G, ebunch=None):
    """networkx.jaccard_coefficient on the GPU: a list of (u, v, p) in ebunch order; ebunch=None: every non-edge, u before
    v in node order (graphs up to MAX_ALL_PAIRS_VERTICES vertices)."""
    return _predict(G, ebunch, "jaccard")


def adamic_adar_index(G, ebunch=None):
    """networkx.adamic_adar_index on the GPU: a list of (u, v, p) in ebunch order; p is the fixed-point sum over 2^32,
    within (common neighbours) * 2^-32 of networkx's float sum."""
    return _predict(G, ebunch, "adamic_adar")


def resource_allocation_index(G, ebunch=None):
    """networkx.resource_allocation_index on the GPU: a list of (u, v, p) in ebunch order; p as in adamic_adar_index."""
    return _predict(G, ebunch, "resource_allocation")


def preferential_attachment(G, ebunch=None):
    """networkx.preferential_attachment on the GPU: a list of (u, v, deg u * deg v) in ebunch order, Python ints."""
    return _predict(G, ebunch, "preferential_attachment")


# ---- candidates ------------------------------------------------------------------------------------------------------
def _candidate_scores(score, num, den):
    return num / (den * (_SCALE if score in _FIXED_POINT else 1.0))


def link_candidates(G, k=10, score="adamic_adar", sources=None):
    """Every source's k best vertices at hop distance exactly two (not the source, not adjacent to it, at least one common
    neighbour) under `score` (one of LINK_SCORES), best first; equal scores rank the smaller vertex id first.
    {'sources' (R,) vertex ids, 'ids' (R, k) int32 vertex ids with -1 in unused slots, 'scores' (R, k) float64, 'num' and
    'den' (R, k) int64: the exact key num / den the ranking uses}.  sources: nodes (default: every vertex).  1 <= k <= 128.
    Vertex ids index CentralityGraph(G).nodes."""
    _check_score(score)

    def run(g):
        rows = np.arange(g.n, dtype=np.int64) if sources is None else _node_ids(g, sources)
        ids, num, den = g.link_candidates(score, k, rows)
        return {"sources": rows, "ids": ids, "scores": _candidate_scores(score, num, den), "num": num, "den": den}
    return _with_graph(G, run)


def _merge_top(sources, ids, num, den, k):
    """The k best pairs (u < v) of per-source candidate lists under the global order -- key num / den descending, then
    (u, v) ascending -- as index arrays (u, v, num, den).  A pair is read from its smaller endpoint's list: the pairs
    through u that beat (u, v) there are pairs that beat it globally, so a pair fewer than k pairs beat is in that list."""
    u = np.repeat(np.asarray(sources, dtype=np.int64), ids.shape[1])
    v, num, den = ids.ravel().astype(np.int64), num.ravel(), den.ravel()
    keep = v > u
    u, v, num, den = u[keep], v[keep], num[keep], den[keep]
    if len(u) > k:   # float division is monotone, so the entries at or above the k-th largest quotient hold the k best
        q = num / den
        keep = q >= np.partition(q, len(q) - k)[len(q) - k]
        u, v, num, den = u[keep], v[keep], num[keep], den[keep]
    if (den == 1).all():
        order = np.lexsort((v, u, -num))
    else:
        rows = list(zip(num.tolist(), den.tolist(), u.tolist(), v.tolist()))

        def compare(a, b):
            left, right = rows[a][0] * rows[b][1], rows[b][0] * rows[a][1]
            if left != right:
                return -1 if left > right else 1
            return -1 if rows[a][2:] < rows[b][2:] else 1
        order = np.array(sorted(range(len(rows)), key=functools.cmp_to_key(compare)), dtype=np.int64)
    order = order[:k]
    return u[order], v[order], num[order], den[order]


def top_links(G, k=10, score="adamic_adar"):
    """The k best non-adjacent pairs of the whole graph under `score`: a list of (u, v, p), u before v in node order, best
    first, equal scores in (u, v) order.  Exact: merged on the host from every vertex's k best candidates.  Pairs without
    a common neighbour are never listed, so fewer than k pairs may come back.  1 <= k <= 128."""
    _check_score(score)

    def run(g):
        ids, num, den = g.link_candidates(score, k, np.arange(g.n, dtype=np.int64))
        u, v, num, den = _merge_top(np.arange(g.n), ids, num, den, int(k))
        nodes = g.nodes
        return [(nodes[a], nodes[b], p) for a, b, p in zip(u.tolist(), v.tolist(), _candidate_scores(score, num, den).tolist())]
    return _with_graph(G, run)


# ---- held-out edges --------------------------------------------------------------------------------------------------
def _spanning_forest_mask(n, edges):
    """True for the edges of a breadth-first spanning forest: one search from an extra vertex tied to every component's
    smallest vertex."""
    from scipy.sparse.csgraph import breadth_first_order, connected_components
    m = len(edges)
    adjacency = sp.coo_matrix((np.ones(m), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    _, labels = connected_components(adjacency, directed=False)
    roots = np.unique(labels, return_index=True)[1]
    rows = np.concatenate([edges[:, 0], np.full(len(roots), n)])
    cols = np.concatenate([edges[:, 1], roots])
    tied = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n + 1, n + 1)).tocsr()
    _, pred = breadth_first_order(tied, n, directed=False, return_predecessors=True)
    child = np.flatnonzero((pred[:n] >= 0) & (pred[:n] < n))
    parent = pred[child].astype(np.int64)
    tree = np.minimum(parent, child) * n + np.maximum(parent, child)
    return np.isin(edges[:, 0] * n + edges[:, 1], tree)


def _split(n, edges, test_fraction, seed, keep_connected):
    if not 0.0 < float(test_fraction) < 1.0:
        raise ValueError("test_fraction must lie in (0, 1)")
    m = len(edges)
    n_test = int(round(float(test_fraction) * m))
    if n_test < 1:
        raise ValueError(f"test_fraction {test_fraction} of {m} edges leaves no test edge")
    rng = np.random.default_rng(seed)
    eligible = np.flatnonzero(~_spanning_forest_mask(n, edges)) if keep_connected else np.arange(m)
    if len(eligible) < n_test:
        raise ValueError(f"{n_test} test edges wanted, but only {len(eligible)} edges lie outside a spanning forest; "
                         "lower test_fraction or pass keep_connected=False")
    if n * (n - 1) // 2 - m < n_test:
        raise ValueError(f"{n_test} negative pairs wanted, but the graph has only {n * (n - 1) // 2 - m} non-edges")
    test = np.sort(rng.choice(eligible, n_test, replace=False))
    hidden = np.zeros(m, dtype=bool)
    hidden[test] = True
    taken = set((edges[:, 0] * n + edges[:, 1]).tolist())
    negatives = []
    while len(negatives) < n_test:   # rejection: a pair is kept when it is no loop, no edge and not drawn before
        draw = np.sort(rng.integers(0, n, size=(2 * (n_test - len(negatives)) + 8, 2)), axis=1)
        for a, b in draw.tolist():
            if a != b and a * n + b not in taken and len(negatives) < n_test:
                taken.add(a * n + b)
                negatives.append((a, b))
    return {"n": n, "train_edges": edges[~hidden], "test_edges": edges[hidden],
            "negative_pairs": np.array(negatives, dtype=np.int64).reshape(-1, 2)}


def split_edges(G, test_fraction=0.1, seed=0, keep_connected=True):
    """Hide round(test_fraction * E) edges for a link-prediction test: {'n', 'train_edges', 'test_edges', 'negative_pairs'},
    (., 2) int64 arrays of vertex ids, u < v.  The test edges are drawn with np.random.default_rng(seed); with
    keep_connected only edges outside a breadth-first spanning forest may be drawn, so the train graph keeps every
    component (ValueError when too few such edges exist).  negative_pairs are as many distinct pairs that are no edges of
    the full graph, drawn by rejection.  Runs on the host."""
    if isinstance(G, CentralityGraph):
        n, edges = G.n, G.edges
    else:
        if hasattr(G, "is_directed") and G.is_directed():
            raise NotImplementedError("link prediction here is for undirected graphs")
        n, edges, _, _ = _graph_arcs(G, None, False)
    return _split(n, edges, test_fraction, seed, keep_connected)


def embedding_link_scores(x, pairs):
    """An embedding's score of every vertex-id pair: minus the squared Euclidean distance, in float64 from the float32
    positions.  x: an embedder or (n, D) positions; pairs: (P, 2) vertex ids."""
    pos = x.positions if hasattr(x, "run_layout") else x
    pos = np.asarray(pos.detach().cpu().numpy() if hasattr(pos, "detach") else pos)
    if pos.ndim != 2:
        raise ValueError(f"positions must be (n, D), got shape {pos.shape}")
    pos = pos.astype(np.float32).astype(np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= len(pos)):
        raise ValueError(f"vertex ids must lie in [0, {len(pos)})")
    d = pos[pairs[:, 0]] - pos[pairs[:, 1]]
    return -np.einsum("ij,ij->i", d, d)


def ranking_auc(pos, neg):
    """The probability that a positive outranks a negative: the exact Mann-Whitney count over all (positive, negative)
    pairs, ties counted one half, then one division.  nan when either side is empty."""
    pos, neg = np.asarray(pos).ravel(), np.sort(np.asarray(neg).ravel())
    if len(pos) == 0 or len(neg) == 0:
        return float("nan")
    below = np.searchsorted(neg, pos, side="left")
    upto = np.searchsorted(neg, pos, side="right")
    twice = int(below.sum()) + int(upto.sum())   # 2 * (below + half the ties)
    return twice / (2 * len(pos) * len(neg))


def average_precision(pos, neg):
    """Average precision of the ranking by descending score: the sum over the distinct score values t, from the top, of
    (recall at t - recall before) * precision at t, where everything scored >= t counts as retrieved -- tied scores
    enter together.  nan without positives."""
    pos, neg = np.asarray(pos).ravel(), np.asarray(neg).ravel()
    if len(pos) == 0:
        return float("nan")
    values = np.unique(np.concatenate([pos, neg]))[::-1]
    spos, sneg = np.sort(pos), np.sort(neg)
    tp = len(pos) - np.searchsorted(spos, values, side="left")
    fp = len(neg) - np.searchsorted(sneg, values, side="left")
    gained = np.diff(np.concatenate([[0], tp]))
    return float(np.sum(gained * (tp / (tp + fp))) / len(pos))


def link_prediction_benchmark(graph_generator, graph_params, dim=3, num_iterations=40, test_fraction=0.1, seed=0,
                              **embedder_kwargs):
    """Held-out-edge link prediction, shaped like run_benchmark: generate the graph, hide test_fraction of its edges
    (split_edges, the train graph keeps its components), embed the train graph, and score the hidden edges and as many
    non-edges with the embedding (embedding_link_scores) and with the five neighbourhood predictors on the train graph.
    {method: {'auc', 'average_precision'}} for every method of LINK_METHODS, plus 'n', 'm', 'n_train', 'n_test',
    'graph_type', 'n_components', the split's arrays, and 'layout_time', 'score_time' (the five predictors) and
    'total_time' in seconds."""
    from . import create_graphem, edges_to_adjacency
    start = time.time()
    n, edges, _ = _generate(graph_generator, graph_params)
    n, edges, _, _ = _graph_arcs(edges, n, False)
    split = _split(n, edges, test_fraction, seed, True)
    pairs = np.concatenate([split["test_edges"], split["negative_pairs"]])
    n_test = len(split["test_edges"])

    embedder = create_graphem(edges_to_adjacency(n, split["train_edges"]), n_components=dim, verbose=False, **embedder_kwargs)
    layout_start = time.time()
    embedder.run_layout(num_iterations=num_iterations)
    layout_time = time.time() - layout_start
    scores = {"embedding": embedding_link_scores(embedder, pairs)}

    score_start = time.time()
    g = CentralityGraph(split["train_edges"], n=n)
    try:
        scores.update({name: values for name, values in _scores(g, pairs).items() if name in LINK_SCORES})
    finally:
        g.close()
    score_time = time.time() - score_start

    result = {name: {"auc": ranking_auc(scores[name][:n_test], scores[name][n_test:]),
                     "average_precision": average_precision(scores[name][:n_test], scores[name][n_test:])}
              for name in LINK_METHODS}
    result.update({"n": n, "m": len(edges), "n_train": len(split["train_edges"]), "n_test": n_test,
                   "graph_type": graph_generator.__name__, "n_components": dim, "train_edges": split["train_edges"],
                   "test_edges": split["test_edges"], "negative_pairs": split["negative_pairs"],
                   "layout_time": layout_time, "score_time": score_time, "total_time": time.time() - start})
    return result
