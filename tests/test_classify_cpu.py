"""Node classification without a GPU: the exported C ABI, the library's host path of gh_qual_knn_vote (device_id = -1) against
the restatement (tests/classify_reference.py) -- ids, votes, class ids and the bits of d2 all equal -- and the Python layer of
graphem-rapids_amd/classify.py; label propagation runs over a stand-in handle that answers from the restatement.  The check_*
helpers take a device id: tests/test_hip_classify.py re-runs them on device 0."""
import ctypes
import os

import networkx as nx
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native, classify

import classify_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_EDGES = np.zeros((0, 2), dtype=np.int32)
SYMBOLS = ["gh_qual_knn_vote", "gh_cent_label_propagation"]
PUBLIC = ["knn_neighbors", "knn_classify", "label_propagation", "split_labels", "accuracy", "confusion_matrix", "macro_f1",
          "node_classification_benchmark", "CLASSIFY_METHODS"]
TILE = 256   # training rows of a staged tile for D <= 16 (csrc/classify.hip KV_TILE_ROWS); D = 17 holds 4096 // 17 = 240
LIST = 32    # entries of a thread's list at most (KV_L): k above it takes another pass; k up to 8 and 16 take lists of 8 and 16


def tile_rows(D):
    return min(TILE, 4096 // D)


def cloud(n, D, seed=0):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


def handle(pos, device_id):
    q = _native.LayoutQuality(NO_EDGES, len(pos), device_id)
    q.set_positions(np.ascontiguousarray(pos, dtype=np.float32))
    return q


def assert_same(got, want):
    for name, g, w in zip(("neighbors", "d2", "pred", "votes"), got, want):
        if w is None:
            assert g is None, name
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.argwhere(g != w)[:5])


def training_set(n, T, classes=4, seed=1):
    rng = np.random.default_rng(seed)
    return rng.permutation(n)[:T], rng.integers(0, classes, T).astype(np.int32)


# D: 17 takes the generic instantiation, 1 too.  T around one tile and two; k at the list-length and pass boundaries.
CASES = ([(D, 5, T) for D in (1, 2, 3, 8, 16, 17) for T in (tile_rows(D) - 1, tile_rows(D), tile_rows(D) + 1, 2 * tile_rows(D) + 1)] +
         [(3, k, T) for k in (1, LIST, LIST + 1, 2 * LIST, 128) for T in (TILE + 1, 2 * TILE + 1)] +
         [(D, k, TILE + 1) for D in (3, 16) for k in (8, 9, 16, 17)] +
         [(16, 128, TILE + 1), (17, LIST + 1, 241), (3, 5, 0), (3, 5, 3), (2, 64, 40)])


def check_case(device_id, D, k, T):
    n = 600
    pos = cloud(n, D, seed=D)
    train, labels = training_set(n, T)
    q = handle(pos, device_id)
    try:
        assert_same(q.knn_vote(k, train, labels), ref.knn(pos, train, labels, None, k))
    finally:
        q.close()


def check_query_inside_training_set(device_id):
    """T = k with the query inside it: k - 1 candidates and one unused slot; outside it: all k."""
    pos = cloud(50, 3)
    train, labels = training_set(50, 5)
    q = handle(pos, device_id)
    try:
        rows = [int(train[2]), int(np.setdiff1d(np.arange(50), train)[0])]
        ids, d2, pred, votes = got = q.knn_vote(5, train, labels, rows)
        assert_same(got, ref.knn(pos, train, labels, rows, 5))
        assert ids[0, 4] == -1 and np.isposinf(d2[0, 4]) and (ids[0, :4] >= 0).all() and rows[0] not in ids[0]
        assert (ids[1] >= 0).all() and sorted(ids[1].tolist()) == sorted(train.tolist())
        # leave-one-out in one call: train = rows = all vertices
        everyone = np.arange(50)
        loo = q.knn_vote(3, everyone, everyone % 3)
        assert_same(loo, ref.knn(pos, everyone, everyone % 3, None, 3))
        assert not (loo[0] == everyone[:, None]).any()
        empty = q.knn_vote(4, [], [], [0, 7])
        assert (empty[0] == -1).all() and np.isposinf(empty[1]).all() and (empty[2] == -1).all() and (empty[3] == 0).all()
    finally:
        q.close()


def lattice(n=300, side=5, seed=5):
    return np.random.default_rng(seed).integers(0, side, size=(n, 2)).astype(np.float32)


def check_lattice(device_id):
    """Small integer coordinates: most distances tie, so the id decides; many points coincide (d2 = 0).  The order of the
    training set changes nothing."""
    pos = lattice()
    assert len(np.unique(pos, axis=0)) <= 25
    train, labels = training_set(300, 150)
    order = np.argsort(train)
    q = handle(pos, device_id)
    try:
        for k in (5, LIST + 1):
            want = ref.knn(pos, train, labels, None, k)
            assert (want[1][:, 0] == 0).sum() > 100
            assert_same(q.knn_vote(k, train, labels), want)
            assert_same(q.knn_vote(k, train[order], labels[order]), want)
            assert_same(q.knn_vote(k, train[order][::-1], labels[order][::-1]), want)
    finally:
        q.close()


def check_overflow(device_id):
    """Coordinates of +-3e38: a difference overflows to +inf, the distances tie there and the id orders them."""
    rng = np.random.default_rng(6)
    pos = (rng.integers(-1, 2, size=(40, 2)) * 3e38).astype(np.float32)
    train, labels = training_set(40, 30)
    q = handle(pos, device_id)
    try:
        want = ref.knn(pos, train, labels, None, 7)
        assert np.isposinf(want[1][want[0] >= 0]).any() and (want[1] == 0).any()
        assert_same(q.knn_vote(7, train, labels), want)
    finally:
        q.close()


def check_votes(device_id):
    """A line: the query at 0, training vertices at distance 1 .. 6."""
    pos = np.arange(7, dtype=np.float32).reshape(-1, 1)
    train = np.arange(1, 7)
    q = handle(pos, device_id)
    try:
        # 2-2-1 at k = 5: the least class of the two with two votes
        ids, _, pred, votes = q.knn_vote(5, train, [9, 9, 4, 4, 7, 4], [0])
        assert ids.tolist() == [[1, 2, 3, 4, 5]] and pred.tolist() == [4] and votes.tolist() == [2]
        _, _, pred, votes = q.knn_vote(6, train, [9, 9, 4, 4, 7, 4], [0])
        assert pred.tolist() == [4] and votes.tolist() == [3]
        # sparse class ids
        _, _, pred, votes = q.knn_vote(4, train, [1_000_000, 7, 1_000_000, 7, 7, 7], [0])
        assert pred.tolist() == [7] and votes.tolist() == [2]
        _, _, pred, votes = q.knn_vote(3, train, [1_000_000, 7, 1_000_000, 7, 7, 7], [0])
        assert pred.tolist() == [1_000_000] and votes.tolist() == [2]
        big = 2 ** 31 - 1
        assert q.knn_vote(1, train, [big] * 6, [0])[2].tolist() == [big]
        # no labels: only the neighbours
        ids, d2, pred, votes = q.knn_vote(2, train, None, [0, 6])
        assert ids.tolist() == [[1, 2], [5, 4]] and d2.tolist() == [[1.0, 4.0], [1.0, 4.0]] and pred is None and votes is None
        # every output left out in turn
        full = q.knn_vote(3, train, train % 2)
        for skip in range(4):
            wanted = [i != skip for i in range(4)]
            part = q.knn_vote(3, train, train % 2, None, *wanted)
            assert part[skip] is None
            assert_same(part, [a if w else None for a, w in zip(full, wanted)])
        assert q.knn_vote(3, train, train % 2, None, False, False, False, False) == (None, None, None, None)
    finally:
        q.close()


def check_rows(device_id):
    pos = cloud(200, 3, seed=2)
    train, labels = training_set(200, 60)
    rng = np.random.default_rng(3)
    q = handle(pos, device_id)
    try:
        full = q.knn_vote(5, train, labels)
        assert_same(full, ref.knn(pos, train, labels, None, 5))
        rows = np.concatenate([rng.permutation(200), rng.integers(0, 200, 50)])
        assert_same(q.knn_vote(5, train, labels, rows), [a[rows] for a in full])
        none = q.knn_vote(5, train, labels, [])
        assert none[0].shape == (0, 5) and none[2].shape == (0,)
    finally:
        q.close()


def check_python_layer(device_id):
    """knn_classify and knn_neighbors on a strided float64 input, any integer labels, both weightings."""
    big = np.random.default_rng(4).standard_normal((120, 6))
    x = big[:, ::2]
    assert x.dtype == np.float64 and not x.flags["C_CONTIGUOUS"]
    pos = np.ascontiguousarray(x.astype(np.float32))
    train, classes = training_set(120, 40, classes=3)
    names = np.array([-5, 40, 7])[classes]   # unsorted, one negative
    order = np.array([-5, 7, 40])
    want = ref.knn(pos, train, np.searchsorted(order, names), None, 5)
    got = gr.knn_classify(x, train, names, k=5, device_id=device_id)
    assert set(got) == {"rows", "pred", "votes", "ids", "d2"} and got["rows"].tolist() == list(range(120))
    assert_same((got["ids"], got["d2"], None, got["votes"]), (want[0], want[1], None, want[3]))
    assert got["pred"].tolist() == order[want[2]].tolist()
    rows = [5, 3, 5]
    some = gr.knn_classify(x, train, names, k=5, rows=rows, device_id=device_id)
    assert some["rows"].tolist() == rows and some["pred"].tolist() == got["pred"][rows].tolist()
    nb = gr.knn_neighbors(x, train, k=5, rows=rows, device_id=device_id)
    assert set(nb) == {"rows", "ids", "d2"} and nb["ids"].tobytes() == want[0][rows].tobytes() and nb["d2"].tobytes() == want[1][rows].tobytes()
    # weights='distance': a coincident training vertex takes all the weight
    line = np.array([[0.0], [0.0], [1.0], [1.5], [2.0]])
    far = gr.knn_classify(line, [1, 2, 3, 4], [3, 8, 8, 8], k=4, rows=[0], device_id=device_id)
    near = gr.knn_classify(line, [1, 2, 3, 4], [3, 8, 8, 8], k=4, rows=[0], weights="distance", device_id=device_id)
    assert far["pred"].tolist() == [8] and far["votes"].tolist() == [3] and near["pred"].tolist() == [3] and near["votes"].tolist() == [1]
    apart = gr.knn_classify(line, [2, 3, 4], [3, 8, 8], k=3, rows=[0], weights="distance", device_id=device_id)
    assert apart["pred"].tolist() == [8]   # 1 / 1 < 1 / 1.5 + 1 / 2
    alone = gr.knn_classify(line, [0], [6], k=2, rows=[0, 1], device_id=device_id)
    assert alone["pred"].tolist() == [-1, 6] and alone["votes"].tolist() == [0, 1]
    for bad in (0, 129, 2.5):
        with pytest.raises(ValueError):
            gr.knn_classify(x, train, names, k=bad, device_id=device_id)
    with pytest.raises(ValueError):
        gr.knn_classify(x, train, names, weights="rank", device_id=device_id)
    with pytest.raises(ValueError):
        gr.knn_classify(x, train, names[:-1], device_id=device_id)


def check_refusals(device_id):
    pos = cloud(30, 3)
    q = _native.LayoutQuality(NO_EDGES, 30, device_id)
    try:
        with pytest.raises(ValueError, match="no positions were set"):
            q.knn_vote(3, [1, 2], [0, 0])
        q.set_positions(pos)
        good = q.knn_vote(3, [1, 2, 9], [0, 1, 1])
        for k in (0, 129, -1):
            with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
                q.knn_vote(k, [1, 2], [0, 0])
        for train, message in (([1, 30, 2], "training row 1 has a vertex id outside [0, n)"), ([1, 2, -1], "training row 2 has a vertex id outside [0, n)"),
                               ([4, 2, 9, 2], "training row 3 repeats vertex 2"), ([5, 5, 30], "training row 1 repeats vertex 5")):
            with pytest.raises(ValueError) as e:
                q.knn_vote(3, train, [0] * len(train))
            assert str(e.value) == message
        with pytest.raises(ValueError) as e:
            q.knn_vote(3, [1, 2, 3], [0, -1, -2])
        assert str(e.value) == "label 1 is negative"
        with pytest.raises(ValueError) as e:
            q.knn_vote(3, [1, 2, 3], [0, 1, 2], [0, 29, 30])
        assert str(e.value) == "row 2 has a vertex id outside [0, n)"
        assert q.lib.gh_qual_knn_vote(q.handle, 3, 0, None, None, 0, None, None, None, _native.ptr(good[2]), None) == _native.GH_ERR_INVALID
        assert_same(q.knn_vote(3, [1, 2, 9], [0, 1, 1]), good)   # a refused call leaves later calls working
        for value in (np.nan, np.inf):
            broken = pos.copy()
            broken[17, 1] = value
            q.set_positions(broken)
            with pytest.raises(ValueError) as e:
                q.knn_vote(3, [1, 2, 9], [0, 1, 1])
            assert str(e.value) == "position row 17 is not finite"
        q.set_positions(pos)
        assert_same(q.knn_vote(3, [1, 2, 9], [0, 1, 1]), good)
    finally:
        q.close()


def check_against_sklearn(device_id):
    """Leave-one-out against KNeighborsClassifier(algorithm='brute') on the queries whose k-th and (k+1)-th float64 squared
    distances differ by more than 1e-4 relatively: at most 5 % of the queries may be left out."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    n, k = 400, 5
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    y = rng.integers(0, 4, n)
    x64 = x.astype(np.float64)
    everyone = np.arange(n)
    ours = {w: gr.knn_classify(x, everyone, y, k=k, weights=w, device_id=device_id)["pred"] for w in ("uniform", "distance")}
    used = 0
    for u in range(n):
        others = everyone[everyone != u]
        dist = np.sort(((x64[others] - x64[u]) ** 2).sum(axis=1))
        if dist[k] - dist[k - 1] <= 1e-4 * dist[k]:
            continue
        used += 1
        for w in ("uniform", "distance"):
            theirs = neighbors.KNeighborsClassifier(k, algorithm="brute", weights=w).fit(x64[others], y[others]).predict(x64[u:u + 1])[0]
            assert ours[w][u] == theirs, (w, u)
    assert used >= 0.95 * n, used


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
    from graphem_rapids_amd import build as gra_build
    header = open(os.path.join(ROOT, "include", "graphem_hip.h")).read()
    assert header.index("---- embedding clusters") < header.index("---- node classification") < header.index("---- edge-list ingestion")
    assert header.index("---- communities") < header.index("---- label propagation") < header.index("---- graph generators")
    gra_build.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS and name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_native.SIGNATURES["gh_qual_knn_vote"][1]) == 11 and len(_native.SIGNATURES["gh_cent_label_propagation"][1]) == 7


def test_null_handle_is_refused_without_a_device():
    lib = _native.load()
    ids = np.zeros(4, dtype=np.int32)
    assert lib.gh_qual_knn_vote(None, 1, 1, _native.ptr(ids), None, 1, _native.ptr(ids), _native.ptr(ids), None, None, None) == _native.GH_ERR_INVALID
    assert lib.gh_qual_last_error(None) == b"handle is NULL"
    assert lib.gh_cent_label_propagation(None, 2, _native.ptr(ids), 3, _native.ptr(ids), None, None) == _native.GH_ERR_INVALID
    assert lib.gh_cent_last_error(None) == b"handle is NULL"


def test_public_names_are_exported():
    for name in PUBLIC:
        assert name in gr.__all__, name
        assert getattr(gr, name) is getattr(classify, name)
    assert "classify" in gr.__all__ and gr.classify is classify
    assert classify.CLASSIFY_METHODS == ("embedding_knn", "label_propagation", "majority")
    assert classify.MAX_NEIGHBORS == 128 and classify.MAX_CLASSES == 1024
    assert callable(_native.LayoutQuality.knn_vote)
    assert callable(gr.CentralityGraph.label_propagation) and callable(_native.CentGraph.label_propagation)


# ---- k-NN on the host path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,T", CASES)
def test_host_path_equals_restatement(D, k, T):
    check_case(-1, D, k, T)


def test_query_inside_the_training_set():
    check_query_inside_training_set(-1)


def test_lattice_ties_and_training_order():
    check_lattice(-1)


def test_overflowing_distances_are_ordered_by_id():
    check_overflow(-1)


def test_vote_ties_sparse_classes_and_null_outputs():
    check_votes(-1)


def test_rows_permuted_repeated_and_null():
    check_rows(-1)


def test_python_layer_on_strided_float64_input():
    check_python_layer(-1)


def test_refusals():
    check_refusals(-1)


def test_against_sklearn():
    check_against_sklearn(-1)


# ---- label propagation -------------------------------------------------------------------------------------------------
class _ReferenceHandle:
    """What _native.CentGraph offers classify.py, answered by the restatement."""

    def __init__(self, n, edges, device_id=0):
        del device_id
        self.n, self.e = int(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2)

    def label_propagation(self, seed_labels, n_classes, max_rounds=100):
        seed_labels = np.asarray(seed_labels)
        assert 1 <= n_classes <= 1024 and seed_labels.min() >= -1 and seed_labels.max() < n_classes
        return ref.propagate(self.n, self.e, seed_labels, max_rounds)

    def close(self):
        pass


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(_native, "CentGraph", _ReferenceHandle)


def path_edges(n):
    return np.column_stack([np.arange(n - 1), np.arange(1, n)])


def ends_seeded(n):
    seeds = np.full(n, -1)
    seeds[0], seeds[-1] = 1, 0
    return seeds


def same_propagation(edges, n, seeds, max_rounds=100):
    """gr.label_propagation equals the restatement; returns the result."""
    got = gr.label_propagation(gr.CentralityGraph(edges, n=n), seeds, max_rounds)
    values = np.unique(np.asarray(seeds)[np.asarray(seeds) >= 0])
    dense = np.full(n, -1)
    dense[np.asarray(seeds) >= 0] = np.searchsorted(values, np.asarray(seeds)[np.asarray(seeds) >= 0])
    labels, rounds, converged = ref.propagate(n, edges, dense, max_rounds)
    want = np.full(n, -1)
    want[labels >= 0] = values[labels[labels >= 0]]
    assert set(got) == {"labels", "rounds", "converged"} and got["labels"].dtype == np.int64
    assert got["labels"].tolist() == want.tolist() and got["rounds"] == rounds and got["converged"] == converged
    return got


def check_paths():
    # 4 vertices: both middles take their seed neighbour's class; 5: the middle vertex sees 1 and 0 once each and takes the least
    assert same_propagation(path_edges(4), 4, ends_seeded(4))["labels"].tolist() == [1, 1, 0, 0]
    got = same_propagation(path_edges(5), 5, ends_seeded(5))
    assert got["labels"].tolist() == [1, 1, 0, 0, 0] and got["converged"] and got["rounds"] == 3
    # the keep rule: a labelled vertex whose class is among the most frequent stays
    kept = same_propagation(path_edges(5), 5, [4, -1, -1, -1, 2])
    assert kept["labels"].tolist() == [4, 4, 2, 2, 2]
    short = same_propagation(path_edges(50), 50, ends_seeded(50), max_rounds=10)
    assert not short["converged"] and short["rounds"] == 10 and (short["labels"][11:39] == -1).all() and short["labels"][10] == 1
    full = same_propagation(path_edges(50), 50, ends_seeded(50))
    assert full["converged"] and (full["labels"] >= 0).all() and full["rounds"] == 25   # 24 rounds to meet, one that changes nothing
    zero = same_propagation(path_edges(50), 50, ends_seeded(50), max_rounds=0)
    assert zero["rounds"] == 0 and not zero["converged"] and zero["labels"].tolist() == ends_seeded(50).tolist()


def check_stars_and_loose_ends():
    star = np.column_stack([np.zeros(5, dtype=np.int64), np.arange(1, 6)])
    assert same_propagation(star, 6, [-1, 3, 3, 3, 8, 8])["labels"][0] == 3       # 3-2
    assert same_propagation(star[:4], 5, [-1, 8, 8, 3, 3])["labels"][0] == 3      # 2-2: the least
    # vertex 6 is isolated, 7-8 a component without a seed; self-loops and duplicate edges in the input
    messy = np.concatenate([star, star[::-1, ::-1], [[2, 2], [0, 0], [7, 8], [8, 7], [7, 7]]])
    got = same_propagation(messy, 9, [-1, 3, 3, 8, 8, 8, -1, -1, -1])
    assert got["labels"].tolist() == [8, 3, 3, 8, 8, 8, -1, -1, -1] and got["converged"]
    everyone = same_propagation(path_edges(6), 6, [2, 0, 1, 1, 0, 2])
    assert everyone["labels"].tolist() == [2, 0, 1, 1, 0, 2] and everyone["rounds"] == 1 and everyone["converged"]
    nobody = gr.label_propagation(path_edges(6), np.full(6, -1))
    assert (nobody["labels"] == -1).all() and nobody["rounds"] == 0
    by_name = gr.label_propagation(nx.relabel_nodes(nx.path_graph(4), {0: "a", 1: "b", 2: "c", 3: "d"}), {"a": 5, "d": 2})
    assert by_name["labels"].tolist() == [5, 5, 2, 2]


def check_hubs_and_class_counts():
    """Vertices of degree 200 and 5000 (lanes stride a row), and 1, 2 and 1024 classes."""
    rng = np.random.default_rng(7)
    for degree, classes in ((200, 2), (5000, 1024), (200, 1)):
        n = degree + 40
        hub = np.column_stack([np.zeros(degree, dtype=np.int64), np.arange(1, degree + 1)])
        tail = np.column_stack([np.arange(degree, n - 1), np.arange(degree + 1, n)])   # a path hanging off the last leaf
        seeds = np.full(n, -1)
        if classes == 1024:
            seeds[1:1025] = rng.permutation(1024)
            seeds[1025:1030] = 1000   # six votes for 1000 against one for every other class; the other leaves follow the hub
        else:
            seeds[1:degree + 1] = rng.integers(0, classes, degree)
        got = same_propagation(np.concatenate([hub, tail]), n, seeds)
        assert got["converged"] and (got["labels"] >= 0).all() and len(np.unique(seeds[seeds >= 0])) == classes
        if classes == 1024:
            assert got["labels"][0] == 1000
    with pytest.raises(ValueError, match="1024"):
        gr.label_propagation(path_edges(1100), np.arange(1100) % 1025)
    with pytest.raises(ValueError):
        gr.label_propagation(path_edges(4), [0, -1, -1, 1], max_rounds=-1)
    with pytest.raises(ValueError):
        gr.label_propagation(path_edges(4), [0, -2, -1, 1])
    with pytest.raises(ValueError):
        gr.label_propagation(path_edges(4), [0, -1, 1])


def test_label_propagation_on_paths(host_only):
    check_paths()


def test_label_propagation_on_stars_and_loose_ends(host_only):
    check_stars_and_loose_ends()


def test_label_propagation_on_hubs_and_class_counts(host_only):
    check_hubs_and_class_counts()


# ---- splits and scores: host code ------------------------------------------------------------------------------------
def test_split_labels():
    labels = np.repeat(np.arange(4), [100, 50, 7, 3])
    labels = np.concatenate([labels, [-1] * 20])
    np.random.default_rng(1).shuffle(labels)
    split = gr.split_labels(labels, 0.1, seed=3)
    train, test = split["train"], split["test"]
    assert set(split) == {"train", "test"} and train.dtype == test.dtype == np.int64
    assert train.tolist() == sorted(train.tolist()) and test.tolist() == sorted(test.tolist())
    assert not set(train.tolist()) & set(test.tolist())
    assert sorted(train.tolist() + test.tolist()) == np.flatnonzero(labels >= 0).tolist()
    assert np.bincount(labels[train]).tolist() == [10, 5, 1, 1]   # max(1, round(0.1 * size))
    again = gr.split_labels(labels, 0.1, seed=3)
    assert np.array_equal(again["train"], train) and np.array_equal(again["test"], test)
    assert not np.array_equal(gr.split_labels(labels, 0.1, seed=4)["train"], train)
    loose = gr.split_labels(labels, 0.1, seed=3, stratified=False)
    assert len(loose["train"]) == 16 and (labels[loose["train"]] >= 0).all() and len(loose["test"]) == 144
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError):
            gr.split_labels(labels, bad)
    nothing = gr.split_labels([-1, -1], 0.5)
    assert len(nothing["train"]) == 0 and len(nothing["test"]) == 0


def test_scores_against_hand_values_and_sklearn():
    y_true = [0, 0, 0, 1, 1, 2, 2, 2, 2, 5]
    y_pred = [0, 0, 1, 1, 2, 2, 2, 2, 0, -1]
    classes, m = gr.confusion_matrix(y_true, y_pred)
    assert classes.tolist() == [-1, 0, 1, 2, 5] and m.dtype == np.int64
    assert m.tolist() == [[0, 0, 0, 0, 0], [0, 2, 1, 0, 0], [0, 0, 1, 1, 0], [0, 1, 0, 3, 0], [1, 0, 0, 0, 0]]
    assert gr.accuracy(y_true, y_pred) == 6 / 10
    # F1 = 2 tp / (2 tp + fp + fn): -1: 0 / 1, 0: 4 / 6, 1: 2 / 4, 2: 6 / 8, 5: 0 / 1
    assert gr.macro_f1(y_true, y_pred) == (0.0 + 4 / 6 + 2 / 4 + 6 / 8 + 0.0) / 5
    assert gr.macro_f1([1, 1], [1, 1]) == 1.0 and gr.accuracy([3], [4]) == 0.0
    assert np.isnan(gr.accuracy([], [])) and np.isnan(gr.macro_f1([], []))
    with pytest.raises(ValueError):
        gr.accuracy([1, 2], [1])
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(2)
    for _ in range(5):
        a, b = rng.integers(0, 6, 200), rng.integers(-1, 5, 200)
        labels = np.union1d(a, b)
        assert np.array_equal(gr.confusion_matrix(a, b)[1], metrics.confusion_matrix(a, b, labels=labels))
        assert gr.accuracy(a, b) == metrics.accuracy_score(a, b)
        assert gr.macro_f1(a, b) == pytest.approx(metrics.f1_score(a, b, labels=labels, average="macro", zero_division=0), abs=1e-15)


BENCHMARK_KEYS = {"embedding_knn", "label_propagation", "majority", "n", "m", "n_train", "n_test", "n_classes", "graph_type",
                  "n_components", "train", "test", "layout_time", "knn_time", "propagation_time", "total_time"}


def majority_by_hand(labels, train, test):
    counts = np.bincount(labels[train])
    return float((labels[test] == int(np.argmax(counts))).mean())
