"""gh_qual_knn_vote and gh_cent_label_propagation (csrc/classify.hip: kv_select_kernel, kv_merge_kernel, lp_round_kernel) on
the device: every case of tests/test_classify_cpu.py against the restatement (tests/classify_reference.py), the device against
the library's host path over many workgroups, several batches and the piece-and-merge path, against itself (a second call, a
second handle), on a live engine's device positions, and label propagation on the real handle.  Every comparison is exact."""
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import classify_reference as ref
from test_classify_cpu import (BENCHMARK_KEYS, CASES, assert_same, check_against_sklearn, check_case, check_hubs_and_class_counts,
                               check_lattice, check_overflow, check_paths, check_python_layer, check_query_inside_training_set,
                               check_refusals, check_rows, check_stars_and_loose_ends, check_votes, cloud, handle,
                               majority_by_hand, path_edges, same_propagation, training_set)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D,k,T", CASES)
def test_device_equals_restatement(D, k, T):
    check_case(0, D, k, T)


def test_query_inside_the_training_set_on_the_device():
    check_query_inside_training_set(0)


def test_lattice_ties_and_training_order_on_the_device():
    check_lattice(0)


def test_overflowing_distances_on_the_device():
    check_overflow(0)


def test_vote_ties_sparse_classes_and_null_outputs_on_the_device():
    check_votes(0)


def test_rows_on_the_device():
    check_rows(0)


def test_python_layer_on_the_device():
    check_python_layer(0)


def test_refusals_on_the_device():
    check_refusals(0)


def test_against_sklearn_on_the_device():
    check_against_sklearn(0)


def both_paths(pos, k, train, labels, rows=None):
    a, b = handle(pos, 0), handle(pos, -1)
    try:
        dev, host = a.knn_vote(k, train, labels, rows), b.knn_vote(k, train, labels, rows)
    finally:
        a.close()
        b.close()
    assert_same(dev, host)
    return dev


def test_device_equals_host_over_many_workgroups_and_batches():
    """n = 70 000, D = 3, T = 7 000, all rows: 274 workgroups of 256 query rows over 28 tiles at k = 10; at k = 128 a batch holds
    2^22 / 128 = 32 768 rows, so the rows go in three batches of four passes each, the last one partial."""
    n = 70_000
    pos = cloud(n, 3)
    train, labels = training_set(n, 7_000, classes=5)
    dev = both_paths(pos, 10, train, labels)
    assert (dev[0] >= 0).all() and dev[3].min() >= 2
    both_paths(pos, 128, train, labels)


def test_few_rows_take_the_piece_and_merge_path():
    """5 rows against T = 60 000: one workgroup of rows, so the 235 tiles are cut into 64 pieces over gridDim.y and merged."""
    n = 61_000
    pos = cloud(n, 3, seed=8)
    train, labels = training_set(n, 60_000, classes=6)
    rows = [17, 60_999, int(train[0]), 30_000, 17]
    for k in (10, 128):
        dev = both_paths(pos, k, train, labels, rows)
        assert_same(dev, ref.knn(pos, train, labels, rows, k))


def test_two_handles_and_two_calls_agree():
    pos = cloud(1061, 3)
    train, labels = training_set(1061, 700)
    want = ref.knn(pos, train, labels, None, 40)
    before = _native.live_allocations()
    a, b = handle(pos, 0), handle(pos, 0)
    for got in (a.knn_vote(40, train, labels), a.knn_vote(40, train, labels), b.knn_vote(40, train, labels)):
        assert_same(got, want)
    assert _native.live_allocations() != before
    a.close()
    b.close()
    assert _native.live_allocations() == before


def live_engine(n=300):
    e = gr.random_regular_edges(n, 4, seed=3)
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    emb = gr.GraphEmbedderHIP(adj + adj.T, n_components=3, verbose=False, seed=0, init="random")
    emb.run_layout(5)
    return emb


def test_live_engine_positions_on_the_device():
    emb = live_engine()
    pos = emb.get_positions().astype(np.float32)
    train, labels = training_set(300, 90)
    want = ref.knn(pos, train, labels, None, 5)
    for got in (gr.knn_classify(emb, train, labels), gr.knn_classify(emb, train, labels, device_id=-1), gr.knn_classify(pos, train, labels, device_id=0)):
        assert_same((got["ids"], got["d2"], got["pred"].astype(np.int32), got["votes"]), want)
    assert gr.knn_neighbors(emb, train)["ids"].tobytes() == want[0].tobytes()


# ---- label propagation on the real handle ------------------------------------------------------------------------------
def test_label_propagation_on_paths_on_the_device():
    check_paths()


def test_label_propagation_on_stars_and_loose_ends_on_the_device():
    check_stars_and_loose_ends()


def test_label_propagation_on_hubs_and_class_counts_on_the_device():
    check_hubs_and_class_counts()


def test_native_label_propagation_refusals():
    g = _native.CentGraph(4, path_edges(4), 0)
    try:
        good = g.label_propagation([0, -1, -1, 1], 2)
        assert good[0].tolist() == [0, 0, 1, 1] and good[1] == 2 and good[2]
        for classes in (0, 1025):
            with pytest.raises(ValueError, match=r"n_classes must lie in \[1, 1024\]"):
                g.label_propagation([0, -1, -1, 0], classes)
        with pytest.raises(ValueError, match="max_rounds"):
            g.label_propagation([0, -1, -1, 1], 2, -1)
        for seeds in ([0, -1, 2, 1], [0, -1, -2, 1]):
            with pytest.raises(ValueError) as e:
                g.label_propagation(seeds, 2)
            assert str(e.value) == "seed label 2 is outside [-1, n_classes)"
        assert g.label_propagation([0, -1, -1, 1], 2)[0].tolist() == good[0].tolist()
        assert g.label_propagation([0, -1, -1, 1], 1024)[0].tolist() == good[0].tolist()
    finally:
        g.close()


def seeded(labels, share, seed):
    rng = np.random.default_rng(seed)
    seeds = np.full(len(labels), -1)
    pick = rng.choice(len(labels), max(1, int(round(share * len(labels)))), replace=False)
    seeds[pick] = labels[pick]
    return seeds


def test_label_propagation_on_a_block_model_and_a_scale_free_graph():
    adjacency, blocks = gr.generate_sbm(75, 4, labels=True)
    edges = np.column_stack(sp.triu(adjacency, k=1).nonzero())
    got = same_propagation(edges, 300, seeded(blocks, 0.1, 0))
    assert got["rounds"] >= 2
    n = 20_000
    edges = gr.barabasi_albert_edges(n, 5, seed=2)
    got = same_propagation(edges, n, seeded(np.random.default_rng(1).integers(0, 7, n), 0.01, 3))
    assert (got["labels"] >= 0).all()


# ---- the benchmark -----------------------------------------------------------------------------------------------------
def test_node_classification_benchmark(monkeypatch):
    made = []
    create = gr.create_graphem
    monkeypatch.setattr(gr, "create_graphem", lambda *a, **kw: made.append(create(*a, **kw)) or made[-1])
    params = {"n_per_block": 60, "num_blocks": 4, "p_in": 0.2, "p_out": 0.01, "labels": True, "seed": 1}
    result = gr.node_classification_benchmark(gr.generate_sbm, params, dim=3, num_iterations=10, train_fraction=0.1, k=5, seed=2)
    assert set(result) == BENCHMARK_KEYS
    adjacency, labels = gr.generate_sbm(**params)
    split = gr.split_labels(labels, 0.1, 2)
    train, test = result["train"], result["test"]
    assert np.array_equal(train, split["train"]) and np.array_equal(test, split["test"])
    assert (result["n"], result["n_train"], result["n_test"], result["n_classes"]) == (240, 24, 216, 4)
    assert result["m"] == adjacency.nnz // 2 and result["graph_type"] == "generate_sbm" and result["n_components"] == 3
    for method in gr.CLASSIFY_METHODS:
        assert set(result[method]) == {"accuracy", "macro_f1"}
    assert result["majority"]["accuracy"] == majority_by_hand(labels, train, test)
    # label propagation equals the restatement's
    seeds = np.full(240, -1)
    seeds[train] = labels[train]
    edges = np.column_stack(sp.triu(adjacency, k=1).nonzero())
    want = ref.propagate(240, edges, seeds, 100)[0]
    assert result["label_propagation"]["accuracy"] == gr.accuracy(labels[test], want[test])
    assert result["label_propagation"]["macro_f1"] == gr.macro_f1(labels[test], want[test])
    # the embedding's accuracy, recomputed by the restatement from the benchmark's embedder's downloaded positions
    assert len(made) == 1 and made[0].n == 240
    pred = ref.knn(made[0].get_positions().astype(np.float32), train, labels[train], test, 5)[2]
    assert result["embedding_knn"]["accuracy"] == gr.accuracy(labels[test], pred)
    assert result["embedding_knn"]["macro_f1"] == gr.macro_f1(labels[test], pred)
