"""gh_qual_kmeans and its siblings (csrc/clusters.hip: cl_lloyd_kernel, cl_finish_kernel, cl_seed_kernel, cl_sums_kernel,
cl_join_kernel) on the device: every case of tests/test_clusters_cpu.py against the restatement of the header's rule
(tests/clusters_reference.py), the device against the library's host path across many workgroups and global-atomic flushes,
on a live engine's device positions, and against itself (a second call, a second handle).  The comparison rule is the CPU
file's: integers and the bits of d2 and of the centres equal; a distance sum of N terms within (N + 2) 2^-53 relative."""
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import clusters_reference as cref
from test_clusters_cpu import (CASES, NO_EDGES, SUM_CASES, assert_same, check_case, check_corners, check_gaussians,
                               check_permuted_and_strided, check_plusplus, check_recovery, check_refusals,
                               check_silhouette_against_sklearn, check_sums, cloud, handle, reference, start_rows)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,D,k", CASES)
def test_device_equals_restatement(n, D, k):
    check_case(0, n, D, k)


def test_gaussians_and_max_iter_on_the_device():
    check_gaussians(0)


def test_rule_corners_on_the_device():
    check_corners(0)


def test_permuted_and_strided_positions_on_the_device():
    check_permuted_and_strided(0)


def test_refusals_on_the_device():
    check_refusals(0)


def test_kmeans_plusplus_on_the_device():
    check_plusplus(0)


@pytest.mark.parametrize("n,D,k,rows", SUM_CASES)
def test_distance_sums_and_silhouette_on_the_device(n, D, k, rows):
    check_sums(0, n, D, k, rows)


def test_silhouette_against_sklearn_on_the_device():
    check_silhouette_against_sklearn(0)


def test_recovery_of_blobs_on_the_device():
    check_recovery(0)


def test_device_equals_host_over_many_workgroups():
    """n = 70 000, D = 3, k = 16, 30 updates at most: 274 workgroups, each flushing its LDS bins with global atomics; and
    k = 600, whose 2400 bins do not fit the workgroup's LDS, so every thread adds to global memory."""
    n = 70_000
    pos = cloud(n, 3)
    for k, max_iter in ((16, 30), (600, 4)):
        start = start_rows(pos, k)
        dev, host = gr.kmeans(pos, k, init=start, max_iter=max_iter, device_id=0), gr.kmeans(pos, k, init=start, max_iter=max_iter, device_id=-1)
        assert_same(dev, host, k)
        assert dev["inertia"] == host["inertia"]
        assert host["n_iter"] == max_iter or host["converged"]
    ids = [gr.kmeans_plusplus(pos, 16, seed=1, device_id=d) for d in (0, -1)]
    assert np.array_equal(ids[0], ids[1])


def test_device_equals_host_when_workgroups_stride():
    """n = 300 001 is more than the 1024 workgroups of a launch hold at once (262 144): some make a second trip, the last one
    partial.  k = 16 keeps the bins in LDS over both trips; k = 1400 walks two centre tiles per trip (a tile holds 1365 at
    D = 3) and adds to the global bins."""
    n = 300_001
    pos = cloud(n, 3)
    for k, max_iter in ((16, 6), (1400, 1)):
        start = start_rows(pos, k)
        dev, host = gr.kmeans(pos, k, init=start, max_iter=max_iter, device_id=0), gr.kmeans(pos, k, init=start, max_iter=max_iter, device_id=-1)
        assert_same(dev, host, k)
        assert host["n_iter"] == max_iter and dev["inertia"] == host["inertia"]


def test_device_sums_equal_host_sums_over_many_tiles():
    """n = 20 000, D = 3: twenty column tiles and a few hundred rows, so the tiles are split over gridDim.y."""
    n, k = 20_000, 9
    pos = cloud(n, 3)
    labels = gr.kmeans(pos, k, max_iter=5, device_id=0)["labels"]
    rows = np.random.default_rng(2).integers(0, n, 300)
    a, b = handle(pos, 0), handle(pos, -1)
    try:
        dev, host = a.cluster_distance_sums(labels, k, rows), b.cluster_distance_sums(labels, k, rows)
    finally:
        a.close()
        b.close()
    # each side is within (N + 2) 2^-53 of the true sum
    assert cref.sums_close(dev, host, 2 * cref.terms(labels, k, rows) + 4)
    assert gr.silhouette_score(pos, labels, exact=False, sample_size=300, device_id=0) == pytest.approx(
        gr.silhouette_score(pos, labels, exact=False, sample_size=300, device_id=-1), abs=4 * (n + 4) * 2.0 ** -53)


def test_two_handles_and_two_calls_agree():
    pos, start, want = reference(1061, 3, 7)
    before = _native.live_allocations()
    a, b = handle(pos, 0), handle(pos, 0)
    first, again, other = a.kmeans(start), a.kmeans(start), b.kmeans(start)
    for got in (first, again, other):
        assert_same(got, want)
    sums = [q.cluster_distance_sums(want["labels"], 7) for q in (a, a, b)]
    assert sums[0].tobytes() == sums[1].tobytes() == sums[2].tobytes()   # no atomics: a run repeats itself
    assert _native.live_allocations() != before
    a.close()
    b.close()
    assert _native.live_allocations() == before


def live_engine(**kw):
    n = 300
    e = gr.random_regular_edges(n, 4, seed=3)
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    emb = gr.GraphEmbedderHIP(adj + adj.T, n_components=3, verbose=False, seed=0, init="random", **kw)
    emb.run_layout(5)
    return emb


def check_live(emb):
    pos = emb.get_positions().astype(np.float32)
    want = cref.kmeans(pos, pos[cref.kmeans_plusplus(pos, 6, 0)])
    for got in (gr.kmeans(emb, 6), gr.kmeans(emb, 6, device_id=-1), gr.kmeans(pos, 6, device_id=0)):
        assert_same(got, want)
    assert np.array_equal(gr.kmeans_plusplus(emb, 6), cref.kmeans_plusplus(pos, 6, 0))
    labels = want["labels"]
    assert np.array_equal(gr.nearest_center(emb, want["centers"])[0], labels)
    assert gr.silhouette_samples(emb, labels).tobytes() == gr.silhouette_samples(pos, labels, device_id=0).tobytes()
    truth = np.arange(emb.n) % 6
    got, same = gr.cluster_recovery(emb, truth, n_init=1), gr.cluster_recovery(pos, truth, n_init=1, device_id=0)
    assert np.array_equal(got["labels"], labels) and got["ari"] == same["ari"] and got["nmi"] == same["nmi"]
    assert got["silhouette"] == same["silhouette"] and got["silhouette_exact"]


def test_live_engine_positions_on_the_device():
    check_live(live_engine())


def test_float64_engine_is_rounded_to_float32():
    import torch
    emb = live_engine(dtype=torch.float64)
    assert emb.get_positions().dtype == np.float64
    check_live(emb)


def test_handle_without_edges_still_answers_the_edge_queries():
    pos = cloud(63, 3)
    q = _native.LayoutQuality(NO_EDGES, 63, 0)
    try:
        q.set_positions(pos)
        assert q.crossings()[1] == 0 and q.kmeans(pos[:3])["converged"]
    finally:
        q.close()
