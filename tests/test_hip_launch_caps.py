"""Every capped launch of the graph analyses on the shared CSR handle, past its cap: graphstats.hip, cores.hip, links.hip,
communities.hip, PageRank of centrality.hip and the frontier kernels that quality.hip's hop profile shares.  A capped grid
covers what does not fit by a loop inside the kernel; the other GPU tests of these files stop at a few thousand vertices
and never take a second trip.  The shapes come from tests/launch_caps.py, where tests/test_launch_caps_cpu.py holds each
of them against the cap as the sources define it: the smallest that pass the cap with a partial last trip.

Expected values at a million vertices come from tests/tiled_graphs.py (tests/test_tiled_graphs_cpu.py proves its argument
on three copies), the others from the restatements the smaller tests use.  Integers are compared exactly, PageRank with
the RTOL and ATOL of tests/test_hip_centrality.py, the hop sums with assert_agree of tests/test_hop_profile_cpu.py."""
import networkx as nx
import numpy as np
import pytest
from scipy.sparse.csgraph import shortest_path

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native

import centrality_reference as cent_ref
import communities_reference as comm_ref
import graphstats_reference as gsr
import launch_caps as lc
import links_reference as links_ref
import tiled_graphs
from test_hip_centrality import ATOL, RTOL
from test_hop_profile_cpu import assert_agree, cloud

pytestmark = pytest.mark.gpu


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


# ---- the vertex, edge and arc loops of graphstats.hip and cores.hip at a million vertices ----------------------------
@pytest.fixture(scope="module")
def million():
    """(expectations, handle): the tiled base of launch_caps.TILED, its shuffled edge list given to the native handle as
    it is (either endpoint first)."""
    t = tiled_graphs.tiled(lc.TILED["base"], lc.TILED["copies"], seed=1)
    g = _native.CentGraph(t.n, t.edges, 0)
    yield t, g
    g.close()


def test_tiled_shape(million):
    t, g = million
    trip = lc.defines().GS_MAX_BLOCKS * lc.defines().GS_BLOCK
    assert g.n == t.n > trip + 256 and g.edges == len(t.canonical) > trip + 256
    assert t.n % 256 and g.edges % 256 and (2 * g.edges) % 256


def test_tiled_components(million):
    """gs_label_init_kernel, gs_hook_kernel, gs_jump_kernel."""
    t, g = million
    labels, count = g.components()
    assert _same(labels, t.labels)
    assert count == len(np.unique(t.labels)) == 28 * t.copies


def test_tiled_triangles(million):
    """gs_triangle_kernel over 2 m arcs."""
    t, g = million
    assert _same(g.triangles(), t.triangles)


def test_tiled_cores(million):
    """cr_degree_kernel, cr_select_kernel and cr_vertex_push_kernel over the vertices."""
    t, g = million
    core, layer, rounds = g.cores()
    assert _same(core, t.core) and _same(layer, t.layer) and rounds == t.rounds == 90
    assert len(np.unique(core)) == 8


def test_tiled_truss(million):
    """cr_upper_count_kernel, cr_edge_id_kernel over the arcs, cr_support_kernel, cr_select_kernel and cr_edge_push_kernel over
    the edges; the values come back in the canonical edge order of the relabelled graph."""
    t, g = million
    truss, rounds = g.truss()
    assert _same(truss, t.truss) and rounds == t.truss_rounds == 33
    assert sorted(set(truss.tolist())) == list(range(2, 10))


def test_tiled_modularity_terms(million):
    """cm_degree_kernel, cm_scatter_T_kernel and cm_numerator_kernel of gh_cent_modularity.  The labelling: the component
    label for half of the vertices, any vertex id for the others."""
    t, g = million
    rng = np.random.default_rng(8)
    labels = np.where(rng.random(t.n) < 0.5, t.labels, rng.integers(0, t.n, size=t.n))
    want = comm_ref.modularity_terms(t.n, t.canonical, labels)
    assert 0 < want[0] < want[2] == 2 * g.edges
    assert g.modularity(labels) == want


# ---- gh_cent_distances: level, fill and seed kernels -----------------------------------------------------------------
def test_distances_many_groups():
    """n = 3000 and 30 000 sources under the default budget: 469 groups in one batch, so a group's row of the level kernel
    gets 4096 / 469 = 8 of the 12 workgroups its vertices need, and the fill kernel takes 469 * 3000 words, the short last
    group's preset bits on its second trip."""
    n, S = lc.LEVEL["n"], lc.LEVEL["sources"]
    G = nx.connected_watts_strogatz_graph(n, 6, 0.1, seed=2)
    D = shortest_path(nx.to_scipy_sparse_array(G, nodelist=range(n), format="csr"), method="D", unweighted=True)
    assert np.isfinite(D).all()
    D = D.astype(np.int64)
    src = np.random.default_rng(3).integers(0, n, size=S)
    src[-1] = src[0]
    g = _native.CentGraph(n, gsr.edge_array(G), 0)
    reached, dist_sum, ecc = g.distances(src)
    g.close()
    assert _same(reached, np.full(S, n, dtype=np.int64))
    assert _same(dist_sum, D.sum(axis=1)[src]) and _same(ecc, D.max(axis=1).astype(np.int32)[src])


def _path_star_isolated():
    """n = 40: the path 0 .. 19, the star of hub 20 with leaves 21 .. 38, the isolated vertex 39."""
    edges = np.array([(v, v + 1) for v in range(19)] + [(20, v) for v in range(21, 39)], dtype=np.int32)
    return lc.SEED["n"], edges


def _sources_with_repeats(n, S, seed):
    src = np.random.default_rng(seed).integers(0, n, size=S)
    src[:n] = np.arange(n)[::-1]   # every vertex, the isolated one first
    src[-1] = 39                   # and last, in the short last group
    return src


def test_distance_seeds_past_the_cap():
    """1 048 576 + 300 sources in one batch of 16 389 groups: gs_frontier_seed_kernel's second trip."""
    n, edges = _path_star_isolated()
    S = lc.SEED["sources"]
    src = _sources_with_repeats(n, S, 4)
    want = gsr.distances(n, edges, np.arange(n))
    g = _native.CentGraph(n, edges, 0)
    got = g.distances(src)
    g.close()
    for have, need in zip(got, want):
        assert _same(have, need[src])
    assert got[0][0] == 1 and got[0][-1] == 1 and set(got[0].tolist()) == {1, 19, 20}


def test_hop_profile_seeds_past_the_cap():
    """The same graph through gh_qual_hop_profile with 524 288 + 300 sources, which seeds with at most 2048 workgroups."""
    n, edges = _path_star_isolated()
    S = lc.HOP_SEED["sources"]
    src = _sources_with_repeats(n, S, 5)
    pos = cloud(n, 2)
    dev, host = gr.hop_profile(pos, edges, sources=src, device_id=0), gr.hop_profile(pos, edges, sources=src, device_id=-1)
    assert_agree(dev, host)
    reached, _, ecc = gsr.distances(n, edges, np.arange(n))
    assert _same(dev["reach"], reached[src] - 1) and _same(dev["eccentricity"], ecc[src])
    assert len(dev["hops"]) == 19 and int(dev["pairs"].sum()) == int((reached[src] - 1).sum())


def test_hop_profile_many_groups():
    """n = 3000, D = 2, 12 000 sources: 188 groups in flight, 2048 / 188 = 10 of the 12 workgroups a group's vertices need."""
    n, S = lc.HOP_LEVEL["n"], lc.HOP_LEVEL["sources"]
    pos, edges = cloud(n, lc.HOP_LEVEL["D"]), gr.random_regular_edges(n, 4, seed=2)
    src = np.random.default_rng(6).integers(0, n, size=S)
    src[-1] = src[0]
    dev, host = gr.hop_profile(pos, edges, sources=src, device_id=0), gr.hop_profile(pos, edges, sources=src, device_id=-1)
    assert_agree(dev, host)
    assert int(host["reach"].min()) == n - 1 and int(host["pairs"].sum()) == S * (n - 1)


# ---- PageRank --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [lc.PAGERANK["step"], lc.PAGERANK["init"]])
def test_pagerank(n):
    """70 001: two rounds of pr_step_kernel, the last a partial one, and 2048 partial sums for the 256 threads of
    pr_check_kernel.  600 001: pr_init_kernel's second trip and ten rounds of the step.  Mean degree 3, so about one vertex
    in twenty is isolated and the dangling sum matters.  The stopping iteration must be the restatement's: the L1 changes
    on both sides of it are held away from n tol, so that no order of summation moves it."""
    edges = gr.erdos_renyi_edges(n, lc.PAGERANK["mean_degree"] / n, seed=n)
    isolated = n - len(np.unique(edges))
    assert n // 40 < isolated < n // 10
    g = _native.CentGraph(n, edges, 0)
    for alpha, tol in [(0.85, 1e-10), (0.5, 1e-9), (0.99, 1e-8)]:
        changes = []
        want, its = cent_ref.pagerank(n, edges, alpha, 1000, tol, changes=changes)
        assert its == len(changes) >= 8
        assert changes[-1] < n * tol * (1 - 1e-6) and changes[-2] > n * tol * (1 + 1e-6)
        x, got_its = g.pagerank(alpha, 1000, tol)
        assert got_its == its
        np.testing.assert_allclose(x, want, rtol=RTOL, atol=ATOL)
    g.close()


# ---- pair scores -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.PAIRS))
def test_pair_scores(name):
    """lk_pair_kernel takes 4096 * 256 / G pairs a trip: 16 384 at 64 lanes a pair (dense130), 131 072 at 8 (ba300)."""
    _, n, e = links_ref.graph(name)
    p = lc.PAIRS[name]
    pairs = np.random.default_rng(9).integers(0, n, size=(p["pairs"], 2))
    pairs = np.concatenate([pairs, [[0, 0], [n - 1, n - 1]], pairs[:1]])
    assert len(pairs) == p["pairs"] + p["extra"] and (pairs[:, 0] == pairs[:, 1]).sum() > 2
    assert len(np.unique(pairs, axis=0)) < len(pairs)
    g = gr.CentralityGraph(e, n=n)
    got = g.link_scores(pairs)
    g.close()
    want = links_ref.pair_scores(n, e, pairs)
    for have, key in zip(got, ("cn", "aa", "ra")):
        assert _same(have, want[key]), key
    assert want["cn"].max() > 0


# ---- Louvain ---------------------------------------------------------------------------------------------------------
def _same_levels(got, want):
    labels, numerators, counts, rounds, M = got
    assert _same(labels, want[0])
    assert (numerators, counts.tolist(), rounds.tolist(), M) == (want[1], list(want[2]), list(want[3]), want[4])


def test_louvain_ring():
    """140 001 short rows: the group-per-row kernels take 131 072 rows a trip.  Every level against the restatement."""
    n, edges = comm_ref.ring(lc.RING["n"])
    want = comm_ref.louvain(n, edges)
    g = _native.CentGraph(n, edges, 0)
    got = g.louvain()
    g.close()
    assert len(want[0]) >= 4
    _same_levels(got, want)


def test_louvain_long_rows():
    """4650 rows, every one longer than CM_SHORT: cm_best_long_kernel has 4096 workgroups, so 554 of them clear their LDS
    table for a second row; 150 hubs of degree >= 1500 do not fit its 1024 slots in the first round and are spilled, by
    workgroups that go on to their next row.  tests/test_launch_caps_cpu.py holds both counts against the degrees.  Two
    levels of eight rounds bound the restatement."""
    n, edges = lc.long_row_graph()
    want = comm_ref.louvain(n, edges, 0, 2, 8)
    g = _native.CentGraph(n, edges, 0)
    got = g.louvain(0, 2, 8)
    g.close()
    assert len(want[0]) == 2 and want[2][0] < n
    _same_levels(got, want)
