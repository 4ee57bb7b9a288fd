"""The rules of include/graphem_hip.h "node classification" and "label propagation", restated in numpy: the float32 distance
chain with explicit np.float32 operations, the k nearest by np.lexsort((ids, d2)) per row, the vote, and the propagation
loop written out.  What tests/test_classify_cpu.py and tests/test_hip_classify.py compare the library against."""
import numpy as np


def d2_chain(x, u, ids):
    """float32 (len(ids),): (((0 + t_0 t_0) + t_1 t_1) + ...), t_d = x[u][d] - x[t][d], every operation a float32 one."""
    x = np.asarray(x, dtype=np.float32)
    s = np.zeros(len(ids), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(x.shape[1]):
            t = np.float32(x[u, d]) - x[ids, d]
            s = s + t * t
    assert s.dtype == np.float32
    return s


def vote(classes):
    """(pred, votes) of the taken neighbours' classes: the greatest count, the least class that reaches it."""
    if len(classes) == 0:
        return -1, 0
    values, counts = np.unique(classes, return_counts=True)
    best = int(counts.max())
    return int(values[counts == best].min()), best


def knn(x, train, labels, rows, k):
    """(neighbors (R, k) int32, d2 (R, k) float32, pred (R,) int32, votes (R,) int32); labels None: pred and votes None."""
    x = np.asarray(x, dtype=np.float32)
    train = np.asarray(train, dtype=np.int64).ravel()
    rows = np.arange(len(x)) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
    class_of = {}
    if labels is not None:
        class_of = dict(zip(train.tolist(), np.asarray(labels).ravel().tolist()))
    ids = np.full((len(rows), k), -1, dtype=np.int32)
    d2 = np.full((len(rows), k), np.inf, dtype=np.float32)
    pred, votes = np.full(len(rows), -1, dtype=np.int32), np.zeros(len(rows), dtype=np.int32)
    for r, u in enumerate(rows.tolist()):
        cand = train[train != u]
        dist = d2_chain(x, u, cand)
        order = np.lexsort((cand, dist))[:k]
        m = len(order)
        ids[r, :m], d2[r, :m] = cand[order], dist[order]
        if labels is not None:
            pred[r], votes[r] = vote(np.array([class_of[t] for t in cand[order].tolist()], dtype=np.int64))
    if labels is None:
        return ids, d2, None, None
    return ids, d2, pred, votes


def canonical_edges(n, edges):
    """(E, 2) int64, u < v, self-loops dropped, duplicates merged."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    assert len(e) == 0 or (e.min() >= 0 and e.max() < n)
    e = np.sort(e, axis=1)
    return np.unique(e, axis=0) if len(e) else e


def propagate(n, edges, seeds, max_rounds):
    """(labels (n,) int32, rounds, converged) of the synchronous rule; seeds: -1 = unlabelled."""
    e = canonical_edges(n, edges)
    seeds = np.asarray(seeds, dtype=np.int64).ravel()
    assert len(seeds) == n
    both = np.concatenate([e, e[:, ::-1]])
    src, dst = both[:, 0], both[:, 1]
    n_classes = max(int(seeds.max()) + 1, 1) if n else 1
    every = np.arange(n)
    cur = seeds.copy()
    it, converged = 0, False
    while it < max_rounds:
        # counts[v][c] = the neighbours w of v with cur[w] == c
        seen = cur[dst]
        counts = np.zeros((n, n_classes), dtype=np.int64)
        np.add.at(counts, (src[seen >= 0], seen[seen >= 0]), 1)
        best = counts.max(axis=1)
        least = counts.argmax(axis=1)   # the first greatest: the least class
        keeps = (cur >= 0) & (counts[every, np.maximum(cur, 0)] == best)
        nxt = np.where((seeds >= 0) | (best == 0) | keeps, cur, least)
        it += 1
        changed = not np.array_equal(nxt, cur)
        cur = nxt
        if not changed:
            converged = True
            break
    return cur.astype(np.int32), it, converged
