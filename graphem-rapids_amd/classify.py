"""Node classification on the GPU: given the labels of a few vertices, predict the rest -- from the embedding by the vote
of the k nearest labelled vertices, and from the graph itself by label propagation.

knn_neighbors and knn_classify run one exact HIP selection over the position snapshot of a layout-quality handle
(csrc/classify.hip: gh_qual_knn_vote; include/graphem_hip.h "node classification"): the k nearest of a SUBSET of the rows
under the total order (float32 squared distance, vertex id), and the vote of their classes.  Ids, votes and the bits of the
distances are a pure function of (positions, train, labels, rows, k): they do not depend on the order of the training set,
on launch geometry, or on whether the kernels or the library's host path (device_id < 0) ran.  It is a float32 rule: a
float64 embedder's positions are rounded to float32 first.

label_propagation is the graph-side baseline (gh_cent_label_propagation; "label propagation"): synchronous rounds with
clamped seeds over the centrality handle's CSR, integers only.

split_labels holds labels out, accuracy, confusion_matrix and macro_f1 score a prediction, and
node_classification_benchmark puts them together: split, embed the whole graph, predict the held-out vertices by the
embedding's neighbours, by label propagation and by the majority class.
"""
import time

import numpy as np

from . import _native
from .centrality import CentralityGraph, _generate
from .clusters import _Points
from .graphstats import _with_graph
from .influence import _graph_arcs

MAX_NEIGHBORS = _native.KNN_MAX_K        # the library's bound on k
MAX_CLASSES = _native.LABEL_MAX_CLASSES  # label propagation's bound on the number of classes
CLASSIFY_METHODS = ("embedding_knn", "label_propagation", "majority")


def _check_k(k):
    if not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"k must be in [1, {MAX_NEIGHBORS}], got {k}")
    return int(k)


def _ids(a, what):
    a = np.asarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be integers")
    return a.astype(np.int64).ravel()


def _rows(p, rows):
    return np.arange(p.q.n, dtype=np.int64) if rows is None else _ids(rows, "rows")


def knn_neighbors(x, train, k=5, rows=None, device_id=None):
    """The k nearest training vertices of every query vertex.  {'rows' (R,) vertex ids, 'ids' (R, k) int32, 'd2' (R, k)
    float32}: nearest first under (float32 squared distance, vertex id); a query never lists itself; unused slots (fewer
    than k candidates) hold -1 and +inf.  x: an embedder, whose device positions are used in place, or (n, D) positions;
    train: distinct vertex ids in any order; rows: vertex ids, any order, repeats allowed (default: every vertex).
    1 <= k <= 128."""
    k = _check_k(k)
    with _Points(x, device_id) as p:
        ids, d2, _, _ = p.q.knn_vote(k, _ids(train, "train"), None, rows if rows is None else _ids(rows, "rows"))
        return {"rows": _rows(p, rows), "ids": ids, "d2": d2}


def _distance_vote(ids, d2, classes_of):
    """(pred, votes) of weights='distance' in float64: the weight of a neighbour is 1 / sqrt(d2); neighbours at distance
    zero take all the weight between them (scikit-learn's rule).  classes_of: class index per vertex.  pred = the least class
    index of greatest weight, -1 without a neighbour; votes = the number of neighbours of that class."""
    R, k = ids.shape
    pred, votes = np.full(R, -1, dtype=np.int64), np.zeros(R, dtype=np.int32)
    for r in range(R):
        taken = ids[r] >= 0
        if not taken.any():
            continue
        cls = classes_of[ids[r][taken]]
        dist = np.sqrt(d2[r][taken].astype(np.float64))
        zero = dist == 0.0
        with np.errstate(divide="ignore"):
            w = zero.astype(np.float64) if zero.any() else 1.0 / dist
        present = np.unique(cls)
        weight = np.array([w[cls == c].sum() for c in present])
        pred[r] = present[int(np.argmax(weight))]   # the first greatest: the least class
        votes[r] = int((cls == pred[r]).sum())
    return pred, votes


def knn_classify(x, train, train_labels, k=5, rows=None, weights="uniform", device_id=None):
    """k-nearest-neighbour classification in the embedding.  {'rows' (R,), 'pred' (R,) labels, 'votes' (R,) int32, 'ids'
    (R, k) int32, 'd2' (R, k) float32}: ids and d2 as in knn_neighbors; with weights='uniform' votes is the greatest number
    of the taken neighbours that share a label and pred the least such label, both from the device; with weights='distance'
    pred is the label of greatest summed weight 1 / distance (float64, on the host from ids and d2; a zero distance takes all
    the weight, as in scikit-learn; the least label on a tie) and votes the number of neighbours that carry it.  A query
    without a candidate gets pred = -1 and votes = 0.  train_labels: any integers, one per training vertex; the output
    carries the same values."""
    k = _check_k(k)
    if weights not in ("uniform", "distance"):
        raise ValueError(f"weights must be 'uniform' or 'distance', got {weights!r}")
    train = _ids(train, "train")
    train_labels = _ids(train_labels, "train_labels")
    if len(train_labels) != len(train):
        raise ValueError(f"{len(train_labels)} labels for {len(train)} training vertices")
    values, inv = np.unique(train_labels, return_inverse=True)   # ascending: the least class index is the least label
    inv = inv.reshape(len(train)).astype(np.int32)
    with _Points(x, device_id) as p:
        uniform = weights == "uniform"
        ids, d2, pred, votes = p.q.knn_vote(k, train, inv, rows if rows is None else _ids(rows, "rows"), pred=uniform, votes=uniform)
        if not uniform:
            classes_of = np.full(p.q.n, -1, dtype=np.int64)
            classes_of[train] = inv
            pred, votes = _distance_vote(ids, d2, classes_of)
        out = np.full(len(pred), -1, dtype=values.dtype if len(values) else np.int64)
        out[pred >= 0] = values[pred[pred >= 0]]
        return {"rows": _rows(p, rows), "pred": out, "votes": votes, "ids": ids, "d2": d2}


# ---- label propagation -----------------------------------------------------------------------------------------------
def _seed_array(g, labels):
    """(n,) int64 with -1 for unknown, from an n-array or a dict node -> label."""
    if isinstance(labels, dict):
        seeds = np.full(g.n, -1, dtype=np.int64)
        if labels:
            nodes = list(labels)
            seeds[g._ids(nodes)] = _ids([labels[v] for v in nodes], "labels")   # pylint: disable=protected-access
        return seeds
    seeds = _ids(labels, "labels")
    if len(seeds) != g.n:
        raise ValueError(f"{len(seeds)} labels for {g.n} vertices")
    return seeds


def _propagate(g, seeds, max_rounds):
    if int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
    if (seeds < -1).any():
        raise ValueError("a label must be -1 (unknown) or >= 0")
    known = seeds >= 0
    values, inv = np.unique(seeds[known], return_inverse=True)
    if len(values) > MAX_CLASSES:
        raise ValueError(f"label propagation holds up to {MAX_CLASSES} classes, got {len(values)}")
    if len(values) == 0:
        return {"labels": seeds.copy(), "rounds": 0, "converged": int(max_rounds) > 0}
    classes = np.full(g.n, -1, dtype=np.int32)
    classes[known] = inv.reshape(-1)
    out, rounds, converged = g.label_propagation(classes, len(values), max_rounds)
    labels = np.full(g.n, -1, dtype=np.int64)
    labels[out >= 0] = values[out[out >= 0]]
    return {"labels": labels, "rounds": rounds, "converged": converged}


def label_propagation(G, labels, max_rounds=100):
    """Synchronous label propagation from the known labels.  {'labels' (n,) int64, -1 where no label arrived, 'rounds',
    'converged'}.  labels: an n-array with -1 for unknown (vertex order of CentralityGraph(G).nodes), or a dict node -> label;
    any integers >= 0, up to 1024 distinct ones.  A labelled vertex never changes.  In a round every other vertex counts the
    labels of its labelled neighbours, keeps its own label when that is among the most frequent and otherwise takes the least
    of the most frequent; all vertices move at once.  The loop ends after a round that changed nothing (converged) or after
    max_rounds rounds.  G: whatever CentralityGraph takes; self-loops are dropped and duplicate edges merged."""
    return _with_graph(G, lambda g: _propagate(g, _seed_array(g, labels), max_rounds))


# ---- held-out labels and scores: host code ---------------------------------------------------------------------------
def split_labels(labels, train_fraction=0.1, seed=0, stratified=True):
    """Hold labels out: {'train', 'test'}, sorted int64 vertex-id arrays that partition the vertices with a label >= 0 (a
    vertex labelled -1 is in neither).  rng = np.random.default_rng(seed).  stratified: the classes in ascending order each
    give max(1, round(train_fraction * size)) training vertices, rng.choice(members, count, replace=False); otherwise
    max(1, round(train_fraction * labelled)) vertices are drawn from all labelled ones."""
    labels = _ids(labels, "labels")
    if not 0.0 < float(train_fraction) < 1.0:
        raise ValueError("train_fraction must lie in (0, 1)")
    known = np.flatnonzero(labels >= 0)
    rng = np.random.default_rng(seed)
    if stratified:
        picks = []
        for c in np.unique(labels[known]):
            members = known[labels[known] == c]
            picks.append(rng.choice(members, max(1, int(round(float(train_fraction) * len(members)))), replace=False))
        train = np.concatenate(picks) if picks else known[:0]
    elif len(known):
        train = rng.choice(known, max(1, int(round(float(train_fraction) * len(known)))), replace=False)
    else:
        train = known
    train = np.sort(train.astype(np.int64))
    return {"train": train, "test": np.setdiff1d(known, train).astype(np.int64)}


def _pair(y_true, y_pred):
    y_true, y_pred = _ids(y_true, "y_true"), _ids(y_pred, "y_pred")
    if len(y_true) != len(y_pred):
        raise ValueError(f"{len(y_true)} true labels and {len(y_pred)} predictions")
    return y_true, y_pred


def accuracy(y_true, y_pred):
    """The share of equal entries: one division of two integers.  nan for empty input."""
    y_true, y_pred = _pair(y_true, y_pred)
    return int((y_true == y_pred).sum()) / len(y_true) if len(y_true) else float("nan")


def confusion_matrix(y_true, y_pred):
    """(classes, matrix): classes = the sorted union of the true and the predicted labels; matrix[i][j] (int64) = how many
    entries of true class classes[i] were predicted as classes[j]."""
    y_true, y_pred = _pair(y_true, y_pred)
    classes, inv = np.unique(np.concatenate([y_true, y_pred]), return_inverse=True)
    inv = inv.reshape(-1)
    c = len(classes)
    matrix = np.bincount(inv[:len(y_true)] * c + inv[len(y_true):], minlength=c * c).reshape(c, c).astype(np.int64)
    return classes, matrix


def macro_f1(y_true, y_pred):
    """The unweighted mean over the union of true and predicted classes of F1 = 2 tp / (2 tp + fp + fn), 0.0 for 0 / 0
    (scikit-learn's f1_score(average='macro', zero_division=0) over the same classes).  nan for empty input."""
    classes, m = confusion_matrix(y_true, y_pred)
    if len(classes) == 0:
        return float("nan")
    tp = np.diag(m)
    den = m.sum(axis=0) + m.sum(axis=1)   # 2 tp + fp + fn
    f1 = [2 * int(t) / int(d) if d else 0.0 for t, d in zip(tp, den)]
    return sum(f1) / len(f1)


def _scores(y_true, y_pred):
    return {"accuracy": accuracy(y_true, y_pred), "macro_f1": macro_f1(y_true, y_pred)}


def _majority(train_labels):
    values, counts = np.unique(train_labels, return_counts=True)
    return values[int(np.argmax(counts))]   # the first greatest: the least label on a tie


def node_classification_benchmark(graph_generator, graph_params, labels=None, dim=3, num_iterations=40, train_fraction=0.1,
                                  k=5, seed=0, **embedder_kwargs):
    """Held-out-label node classification, shaped like link_prediction_benchmark: generate the graph (the generator returns
    a graph, or (graph, labels) as generate_sbm(labels=True) does; `labels` overrides), split the labels (split_labels,
    stratified), embed the WHOLE graph, and predict the test vertices by the methods of CLASSIFY_METHODS: 'embedding_knn'
    (knn_classify with k neighbours on the embedder's device positions), 'label_propagation' on the graph (a vertex no label
    reaches counts as wrong) and 'majority' (the most common training label, the least on a tie).
    {method: {'accuracy', 'macro_f1'}}, plus 'n', 'm', 'n_train', 'n_test', 'n_classes', 'graph_type', 'n_components',
    'train', 'test', and 'layout_time', 'knn_time', 'propagation_time' and 'total_time' in seconds."""
    from . import create_graphem, edges_to_adjacency
    start = time.time()
    params = dict(graph_params)
    out = graph_generator(**params)
    if isinstance(out, tuple):
        graph, made = out[0], out[1]
        labels = made if labels is None else labels
    else:
        graph = out
    if labels is None:
        raise ValueError("no labels: pass labels=, or a generator that returns (graph, labels)")
    n, edges, _ = _generate(lambda **_: graph, params)   # the graph in hand, read as run_benchmark reads a generator's
    labels = _ids(labels, "labels")
    n, edges, _, _ = _graph_arcs(edges, max(n, len(labels)), False)
    if len(labels) != n:
        raise ValueError(f"{len(labels)} labels for {n} vertices")
    split = split_labels(labels, train_fraction, seed, True)
    train, test = split["train"], split["test"]
    truth = labels[test]

    embedder = create_graphem(edges_to_adjacency(n, edges), n_components=dim, verbose=False, **embedder_kwargs)
    layout_start = time.time()
    embedder.run_layout(num_iterations=num_iterations)
    layout_time = time.time() - layout_start

    knn_start = time.time()
    pred = {"embedding_knn": knn_classify(embedder, train, labels[train], k=k, rows=test)["pred"]}
    knn_time = time.time() - knn_start

    propagation_start = time.time()
    seeds = np.full(n, -1, dtype=np.int64)
    seeds[train] = labels[train]
    g = CentralityGraph(edges, n=n)
    try:
        pred["label_propagation"] = _propagate(g, seeds, 100)["labels"][test]
    finally:
        g.close()
    propagation_time = time.time() - propagation_start
    pred["majority"] = np.full(len(test), _majority(labels[train]) if len(train) else -1, dtype=np.int64)

    result = {name: _scores(truth, pred[name]) for name in CLASSIFY_METHODS}
    result.update({"n": n, "m": len(edges), "n_train": len(train), "n_test": len(test),
                   "n_classes": len(np.unique(labels[labels >= 0])), "graph_type": graph_generator.__name__, "n_components": dim,
                   "train": train, "test": test, "layout_time": layout_time, "knn_time": knn_time,
                   "propagation_time": propagation_time, "total_time": time.time() - start})
    return result
