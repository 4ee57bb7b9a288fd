"""gh_qual_* (csrc/quality.hip) on the device: against the restatement of the header's rule (tests/quality_reference.py)
bit for bit on the CPU grid, against the library's host path where dozens of column tiles and a last partial tile are in
play, on a live engine's device positions, and against itself (rows, the estimator, a second handle, a second call)."""
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import quality_reference as ref
from conftest import load_golden
from test_quality_cpu import (CASES, DISJOINT_BOXES, check_against_restatement, check_estimator, check_lengths, check_rows,
                              gaussian, grid_graph)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(name):
    check_against_restatement(0, name)


def both_paths(pos, edges):
    out = []
    for device_id in (-1, 0):
        q = _native.LayoutQuality(edges, len(pos), device_id)
        q.set_positions(pos)
        out.append((q.crossings(), q.edge_lengths()))
        q.close()
    return out


def test_device_equals_host_over_dozens_of_tiles():
    """E = 12001: twelve column tiles of 1024 with a last one of 737, 47 row workgroups with a last one of 225 rows."""
    pos, edges = gaussian(12001)
    ((want, want_sum), want_len), ((got, got_sum), got_len) = both_paths(pos, edges)
    assert np.array_equal(got, want) and got_sum == want_sum > 0
    check_lengths(got_len, ref.length_sums(pos, edges), len(edges))
    assert np.array_equal(got_len[:2], want_len[:2])


def test_device_equals_host_on_a_grid_with_chords():
    """A 110 x 110 grid drawn on its lattice (no crossings: touching at shared vertices, collinear neighbours) plus 200 long
    random chords, which cross many grid edges and each other."""
    pos, edges = grid_graph(110)
    rng = np.random.default_rng(9)
    edges = np.concatenate([edges, rng.integers(0, len(pos), (200, 2)).astype(np.int32)])
    ((want, want_sum), _), ((got, got_sum), _) = both_paths(pos, edges)
    assert np.array_equal(got, want) and got_sum == want_sum
    assert want[:-200].sum() > 0 and want[-200:].max() > 50


def test_disjoint_bounding_boxes_cross_on_the_device_too():
    assert gr.edge_crossing_counts(DISJOINT_BOXES, np.array([[0, 1], [2, 3]]), device_id=0).tolist() == [1, 1]


@pytest.fixture(scope="module")
def live():
    g = load_golden("c1_er1000")
    e, n = g["edges"], int(g["n"])
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    emb = gr.GraphEmbedderHIP(adj + adj.T, n_components=3, verbose=False, seed=0, init="random")
    emb.run_layout(3)
    return emb


def test_live_engine_positions_on_the_device(live):
    pos = live.get_positions()
    want = ref.crossing_counts(pos, live._edges_np)   # pylint: disable=protected-access
    total = int(want.sum()) // 2
    assert live.edge_crossings() == total > 0
    assert live.edge_crossings() == total
    assert np.array_equal(gr.edge_crossing_counts(live), want)
    assert gr.edge_crossings(pos, live.adjacency) == total          # the (positions, adjacency) form: the embedder's edge ids
    assert np.array_equal(gr.edge_crossing_counts(pos, live.adjacency), want)
    out = live.layout_quality()
    assert out["crossings"] == total and out["crossings_exact"] and out["L_min"] == live.L_min and out["n_edges"] == live.n_edges
    assert out == {**gr.layout_quality(pos, live._edges_np), "L_min": live.L_min}   # pylint: disable=protected-access
    est = live.edge_crossings(sample_size=512, seed=4)
    assert est == gr.estimate_edge_crossings(pos, live._edges_np, sample_size=512, seed=4, device_id=-1)   # pylint: disable=protected-access


def test_snapshot_outlives_further_iterations(live):
    engine = live._engine   # pylint: disable=protected-access
    q = _native.LayoutQuality(live._edges_np, live.n, live.device.index)   # pylint: disable=protected-access
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    before = ref.crossing_counts(live.get_positions(), live._edges_np)   # pylint: disable=protected-access
    live.run_layout(1)
    assert np.array_equal(q.crossings()[0], before)
    after = ref.crossing_counts(live.get_positions(), live._edges_np)   # pylint: disable=protected-access
    assert not np.array_equal(after, before)
    q.set_positions_device(engine.positions_unpadded_device_ptr(), engine.D)
    assert np.array_equal(q.crossings()[0], after)
    q.close()


def test_float64_engine_is_rounded_to_float32():
    g = load_golden("rr200_s64")
    e, n = g["edges"], int(g["n"])
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    import torch
    emb = gr.GraphEmbedderHIP(adj + adj.T, n_components=2, verbose=False, seed=0, init="random", dtype=torch.float64)
    emb.run_layout(2)
    pos = emb.get_positions()
    assert pos.dtype == np.float64
    want = ref.crossing_counts(pos.astype(np.float32), emb._edges_np)   # pylint: disable=protected-access
    assert emb.edge_crossings() == int(want.sum()) // 2


def test_rows_on_the_device():
    check_rows(0)
    check_rows(0, "golden_pos_final")


def test_estimator_on_the_device():
    check_estimator(0)


def test_two_handles_agree():
    pos, edges = gaussian(5051)
    a, b = _native.LayoutQuality(edges, len(pos), 0), _native.LayoutQuality(edges, len(pos), 0)
    a.set_positions(pos)
    b.set_positions(pos)
    first, again, other = a.crossings(), a.crossings(), b.crossings()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[0], other[0]) and first[1] == again[1] == other[1]
    assert np.array_equal(a.edge_lengths(), b.edge_lengths())
    a.close()
    b.close()
