"""gh_qual_hop_profile (csrc/quality.hip, qual_hop_level_kernel and qual_hop_reduce_kernel) on the device: every case of
tests/test_hop_profile_cpu.py against the restatement of the header's rule (tests/hops_reference.py), the device against
the library's host path where many source groups, many workgroups per group, a short last group and thousands of levels
are in play, on a live engine's device positions, and against itself (a second call, a second handle).  The comparison rule
is the CPU file's: integers and min / max bits equal, a double sum of N terms within (N + 8) 2^-52 relative."""
import numpy as np
import pytest
import scipy.sparse as sp

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import graphstats_reference as gsref
from conftest import load_golden
from test_hop_profile_cpu import (CASES, GRAPHS, assert_agree, check_case, check_coincident, check_distance_quality, check_measures,
                                  check_non_finite, check_strided, cloud, graph, reference, rel, same_exact_part)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,D", CASES)
def test_device_equals_restatement(name, D):
    check_case(0, name, D)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_coincident_points_on_the_device(name):
    check_coincident(0, name)


def test_strided_positions_on_the_device():
    check_strided(0)


def test_non_finite_rows_on_the_device():
    check_non_finite(0)


def test_measures_on_the_device():
    check_measures(0)


def test_distance_quality_on_the_device():
    check_distance_quality(0)


def test_device_equals_host_over_many_groups():
    """n = 12001, d = 8, D = 3, 700 random sources: 11 groups with a last one of 60, 47 workgroups to a group, and the slab
    reduction over all 517 of them."""
    n = 12001
    pos, edges = cloud(n, 3), gr.random_regular_edges(n, 8, seed=1)
    src = np.random.default_rng(5).integers(0, n, 700)
    dev, host = gr.hop_profile(pos, edges, sources=src, device_id=0), gr.hop_profile(pos, edges, sources=src, device_id=-1)
    assert_agree(dev, host)
    assert int(host["reach"].min()) == n - 1 and 4 <= len(host["hops"]) <= 8 and int(host["pairs"].sum()) == 700 * (n - 1)


def test_device_equals_host_over_thousands_of_levels():
    """A permuted path of 5000 with 70 sources: a second group of 6, and as many levels as the farthest source needs."""
    n = 5000
    pos, edges = cloud(n, 2), gsref.permuted_path(n)
    src = np.random.default_rng(6).integers(0, n, 70)
    dev, host = gr.hop_profile(pos, edges, sources=src, device_id=0), gr.hop_profile(pos, edges, sources=src, device_id=-1)
    assert_agree(dev, host)
    assert len(host["hops"]) == int(host["eccentricity"].max()) > 2500 and np.array_equal(host["reach"], np.full(70, n - 1))


def test_unstaged_source_rows_over_many_workgroups():
    """D = 130: the source rows are read from memory; n = 3000 gives twelve workgroups to a group."""
    n = 3000
    pos, edges = cloud(n, 130), gr.random_regular_edges(n, 4, seed=2)
    src = np.random.default_rng(7).integers(0, n, 100)
    assert_agree(gr.hop_profile(pos, edges, sources=src, device_id=0), gr.hop_profile(pos, edges, sources=src, device_id=-1))


def test_two_handles_and_two_calls_agree():
    n, edges, _ = graph("regular")
    pos, want = reference("regular", 3)
    start = _native.live_allocations()
    a, b = _native.LayoutQuality(edges, n, 0), _native.LayoutQuality(edges, n, 0)
    a.set_positions(pos)
    b.set_positions(pos)
    first, again, other = a.hop_profile(), a.hop_profile(), b.hop_profile()
    for key in ("pairs", "reach", "eccentricity", "min_d2", "max_d2"):
        assert first[key].tobytes() == again[key].tobytes() == other[key].tobytes(), key
        assert first[key].tobytes() == want["all"][key].tobytes(), key
    assert _native.live_allocations() != start
    a.close()
    b.close()
    assert _native.live_allocations() == start


def test_hop_profile_and_cent_distances_share_one_search():
    """gh_qual_hop_profile and gh_cent_distances run the same frontier step (csrc/frontier_core.h).  n = 130: a path of 66, a
    star whose hub 66 has 62 leaves, and the isolated vertex 129; 65 sources -- two groups, the last one of one source --
    with the hub twice and the isolated vertex.  The hop profile counts the pairs at hop >= 1, gh_cent_distances the source
    too (tests/hops_reference.py, tests/graphstats_reference.py): reach = reached - 1, and the eccentricities are equal."""
    n = 130
    edges = np.array([(v, v + 1) for v in range(65)] + [(66, v) for v in range(67, 129)], dtype=np.int32)
    src = np.r_[np.arange(0, 124, 2), 129, 66, 5]
    assert len(src) == 65 and len(edges) == 65 + 62
    hops = gr.hop_profile(cloud(n, 2), edges, sources=src, device_id=0)
    g = _native.CentGraph(n, edges, 0)
    reached, _, ecc = g.distances(src)
    g.close()
    assert hops["reach"].dtype == reached.dtype == np.int64 and hops["eccentricity"].dtype == ecc.dtype == np.int32
    assert np.array_equal(hops["reach"], reached - 1) and np.array_equal(hops["eccentricity"], ecc)
    on_path = src < 66
    assert np.array_equal(reached[on_path], np.full(on_path.sum(), 66)) and np.array_equal(ecc[on_path], np.maximum(src, 65 - src)[on_path])
    assert reached[62] == 1 and ecc[62] == 0 and reached[63] == reached[33] == 63 and ecc[63] == ecc[33] == 1 and src[33] == 66


def live_engine(**kw):
    n = 300
    e = gr.random_regular_edges(n, 4, seed=3)
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    emb = gr.GraphEmbedderHIP(adj + adj.T, n_components=3, verbose=False, seed=0, init="random", **kw)
    emb.run_layout(5)
    return emb


def check_live(emb):
    pos = emb.get_positions().astype(np.float32)
    edges = emb._edges_np   # pylint: disable=protected-access
    assert_agree(gr.hop_profile(emb), gr.hop_profile(pos, edges, device_id=0))
    assert same_exact_part(gr.hop_profile(emb), gr.hop_profile(pos, edges, device_id=-1))
    got, want = gr.distance_quality(emb), gr.distance_quality(pos, edges, device_id=0)
    assert list(got) == list(want)
    for key in ("n_sources", "exact", "pairs", "n_unreachable", "max_hop", "stress_stderr"):
        assert got[key] == want[key], key
    assert got["n_sources"] == emb.n and got["exact"] is True and np.array_equal(got["hops"], want["hops"])
    # the two calls sum the same terms, so each sum agrees within the rule; the measures are held as in the CPU file, at 1e-12
    for key in ("stress", "scale", "correlation", "mean_d"):
        assert rel(got[key], want[key]), key


def test_live_engine_positions_on_the_device():
    check_live(live_engine())


def test_float64_engine_is_rounded_to_float32():
    import torch
    emb = live_engine(dtype=torch.float64)
    assert emb.get_positions().dtype == np.float64
    check_live(emb)


def test_golden_graph_on_a_live_engine():
    g = load_golden("c1_er1000")
    e, n = g["edges"], int(g["n"])
    adj = sp.csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    emb = gr.GraphEmbedderHIP(adj + adj.T, n_components=3, verbose=False, seed=0, init="random")
    emb.run_layout(3)
    dev = gr.hop_profile(emb, sources=np.arange(0, n, 7))
    host = gr.hop_profile(emb.get_positions().astype(np.float32), emb._edges_np, sources=np.arange(0, n, 7), device_id=-1)   # pylint: disable=protected-access
    assert_agree(dev, host)
    assert dev["n_unreachable"] == host["n_unreachable"]
