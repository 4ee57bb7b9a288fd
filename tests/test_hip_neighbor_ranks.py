"""gh_qual_neighbor_ranks (csrc/quality.hip, qual_rank_kernel) on the device: every case of tests/test_neighbor_ranks_cpu.py
against the restatement of the header's rule (tests/neighbors_reference.py), the device against the library's host path
where many column tiles, a last partial tile and the split of the columns over workgroups are in play, on a live engine's
device positions, and against itself (a second call, a second handle).  All comparisons are for equality."""
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import neighbors_reference as ref
from conftest import load_golden
from test_neighbor_ranks_cpu import (ARRAYS, CASES, assert_same, check_against_restatement, check_measures, check_rows,
                                     check_strided, cloud, planted, reference)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_restatement(name):
    check_against_restatement(0, name)


def test_strided_positions_on_the_device():
    check_strided(0)


def test_rows_on_the_device():
    check_rows(0)
    check_rows(0, "hub")


def test_measures_on_the_device():
    check_measures(0)
    pos, edges = planted()
    assert gr.link_auc(pos, edges, device_id=0) == 1.0
    assert gr.neighborhood_preservation(pos, edges, device_id=0) == {"precision": 1.0, "jaccard": 1.0}


@pytest.fixture(scope="module")
def big():
    """n = 12001, D = 3, random-regular d = 8: twelve column tiles of 1024 with a last one of 737."""
    n = 12001
    return cloud(n), gr.random_regular_edges(n, 8, seed=1)


def test_device_equals_host_over_many_tiles(big):
    """All rows: 12001 pieces, 3001 workgroups, every workgroup walks all twelve tiles."""
    pos, edges = big
    want = gr.neighbor_ranks(pos, edges, device_id=-1)
    assert_same(gr.neighbor_ranks(pos, edges, device_id=0), want)
    assert want["below"].max() > 5000 and np.array_equal(np.diff(want["indptr"]), np.full(len(pos), 8))


def test_device_equals_host_with_split_columns(big):
    """37 rows: ten workgroups, so the twelve tiles are split over gridDim.y and the partial counts are added by the second
    launch."""
    pos, edges = big
    rows = np.random.default_rng(5).integers(0, len(pos), 37)
    assert_same(gr.neighbor_ranks(pos, edges, rows=rows, device_id=0), gr.neighbor_ranks(pos, edges, rows=rows, device_id=-1))


def test_hub_with_few_rows_splits_columns_too():
    """The hub's 79 pieces alone: twenty workgroups over six tiles of 1024 columns."""
    pos, edges, want = reference("hub")
    got = gr.neighbor_ranks(pos, edges, rows=[0, 5999, 0], device_id=0)
    lo, hi = want["indptr"][0], want["indptr"][1]
    assert np.array_equal(got["below"][:5000], want["below"][lo:hi]) and np.array_equal(got["equal"][:5000], want["equal"][lo:hi])
    assert np.array_equal(got["below"][-5000:], want["below"][lo:hi]) and ref.same_bits(got["dist2"][:5000], want["dist2"][lo:hi])


def test_two_handles_and_two_calls_agree():
    pos, edges, want = reference("ladder")
    a, b = _native.LayoutQuality(edges, len(pos), 0), _native.LayoutQuality(edges, len(pos), 0)
    a.set_positions(pos)
    b.set_positions(pos)
    first, again, other = a.neighbor_ranks(), a.neighbor_ranks(), b.neighbor_ranks()
    for x, y, z, key in zip(first, again, other, ARRAYS[1:]):
        assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, want[key]), key
    a.close()
    b.close()


def live_engine(case, **kw):
    g = load_golden(case)
    e, n = g["edges"], int(g["n"])
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    emb = gr.GraphEmbedderHIP(adj + adj.T, verbose=False, seed=0, init="random", **kw)
    emb.run_layout(3)
    return emb


def check_live(emb):
    pos = emb.get_positions().astype(np.float32)
    edges = emb._edges_np   # pylint: disable=protected-access
    want = ref.neighbor_ranks(pos, edges)
    assert_same(gr.neighbor_ranks(emb), want)
    out = emb.embedding_quality()
    assert out == gr.embedding_quality(emb) == gr.embedding_quality(pos, edges, device_id=-1)
    assert out["n_vertices"] == emb.n and out["sources_exact"] is True
    assert out["link_auc"] == ref.link_auc(pos, edges) and out["neighborhood_precision"] == ref.neighborhood_preservation(pos, edges)[0]
    assert list(emb.layout_quality())[:2] == ["n_edges", "crossings"]


def test_live_engine_positions_on_the_device():
    check_live(live_engine("c1_er1000", n_components=3))


def test_float64_engine_is_rounded_to_float32():
    import torch
    emb = live_engine("c1_er1000", n_components=3, dtype=torch.float64)
    assert emb.get_positions().dtype == np.float64
    check_live(emb)
