"""The searches knn_method='auto' takes by itself -- the grid (csrc/grid_core.h) and the exact inverted file (csrc/ivf.hip)
-- on the states where a search goes wrong, against the oracle and the fused scan.  README and DESIGN section 8 say both
return the scan's neighbour rows id for id, ties on the smaller (caller's) edge id; the existing tests of the two
searches use Gaussian clouds and a few outliers only.  Here:

  1. degenerate states (collapsed, lattice, flat axis, a majority of coincident queries, a layout 200 iterations in,
     queries whose six grid rings hold fewer than K midpoints, hubs, clouds scaled by 1e-4 and 1e4) under every search,
     with vertex reordering off and on (reordering renumbers the vertices, so a wrong edge-id mapping shows in the
     tie-breaks): rows = oracle = scan engine, one step within 1e-4 of the oracle and 2e-6 of the scan engine;
  2. clusters of coincident midpoints that make candidate lists of 8 K - 16 K keys, lists past the 16384 cap (the
     exhaustive search), and the inverted file's LDS buffers (see test_ivf_buffers_of_a_tile_overflow);
  3. k at the limits of the register extraction (K = k + 1 = 128) and past it;
  4. the approximate inverted file on states where most lists are empty: what a row is, if not exact;
  5. the next iteration's set-up done inside the normalise launch, invalidated by caller ids, for grid and inverted file;
  6. device-sampled runs through each search, and the public class's 'auto' choice;
  7. the grid on row partitions of a collapsed state;
  and non-finite positions for the grid (rows against the scan engine; queries with an infinite coordinate are flagged
  in the overflow counters and searched exhaustively).

Non-finite positions under the inverted file are out of scope: its f16 assignment and minima (ivf.hip, the note at
ivf_half) assume finite coordinates.

Needs a real MI355X."""
import functools
import zlib

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, DEG, K = 60000, 8, 10          # 240 000 edges: each search really runs (grid: >= 16384 edges, inverted file: >= 4096)
S = 1024
SEARCHES = {
    "scan": dict(knn_method="scan"),
    "grid": dict(knn_method="grid"),
    "ivf_exact": dict(knn_method="ivf", ivf_probes=-1),
    "ivf_all": dict(knn_method="ivf", ivf_lists=128, ivf_probes=128),   # every list probed
}
KERNEL = {"grid": "grid_build", "ivf_exact": "ivf_scan", "ivf_all": "ivf_scan"}


@functools.lru_cache(maxsize=None)
def _edges():
    import graphem_rapids_amd as gra
    return np.ascontiguousarray(gra.random_regular_edges(N, DEG, seed=31), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _hub_edges():
    """The graph of test_hip_parity.test_skewed_degrees_hubs: hubs of degree 20000, 2000 and 600 on a 4-regular graph."""
    import graphem_rapids_amd as gra
    n = 50000
    rng = np.random.default_rng(11)
    base = gra.random_regular_edges(n, 4, seed=9).astype(np.int64)
    extra = []
    for hub, deg in ((17, 20000), (4021, 2000), (49999, 600)):
        nb = rng.choice(n, size=deg, replace=False)
        nb = nb[nb != hub]
        extra.append(np.stack([np.minimum(hub, nb), np.maximum(hub, nb)], axis=1))
    e = np.unique(np.concatenate([np.sort(base, axis=1)] + extra), axis=0)
    return np.ascontiguousarray(e, dtype=np.int32)


def _searches(D):
    return [s for s in SEARCHES if s != "grid" or D <= 3]


@functools.lru_cache(maxsize=None)
def _iter200(D):
    """The scan engine's positions after 200 device-sampled iterations from the reference's start 0.1 N(0, 1)."""
    from graphem_rapids_amd import _native
    pos = (np.random.default_rng(200 + D).standard_normal((N, D)) * 0.1).astype(np.float32)
    eng = _native.Engine(N, D, _edges(), 1.0, 0.2, 0.5, K, 256, seed=3, knn_method="scan")
    eng.set_positions(pos)
    eng.run(200)
    out = eng.get_positions()
    eng.close()
    return out


def _cluster(pos, edges, members, point):
    """Move `members` onto one point; the edges with both ends among them (their midpoints coincide)."""
    pos[members] = np.float32(point)
    inside = np.isin(edges[:, 0], members) & np.isin(edges[:, 1], members)
    return np.nonzero(inside)[0]


def _case(kind, D, S=S):
    """(n, edges, positions, sampled edge ids) of a named state."""
    edges = _hub_edges() if kind == "hubs" else _edges()
    n = int(edges.max()) + 1 if kind == "hubs" else N
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{D}".encode()))
    pos = rng.standard_normal((n, D)).astype(np.float32)
    sampled = rng.permutation(len(edges))[:S].astype(np.int32)
    if kind == "collapsed":        # duplicated positions, a third of the graph on one point: ~27 K coincident midpoints
        pos *= np.float32(0.1)
        pos[1::2] = pos[0::2]
        pos[: n // 3] = pos[7]
    elif kind == "lattice":        # integer coordinates: distances tie everywhere, points on cell and list boundaries
        pos = rng.integers(-2, 3, size=(n, D)).astype(np.float32)
    elif kind == "flat_axis":      # one coordinate always 0: that axis has an inter-quartile range of 0
        pos[:, 2] = 0.0
    elif kind == "majority":       # >= 80 % of the queries on one point: the grid frame's IQR is 0 on every axis
        inside = _cluster(pos, edges, rng.permutation(n)[: n // 10], 0.5)
        m = int(0.85 * S)
        sampled[:m] = rng.permutation(inside)[:m]
        sampled[m:] = rng.permutation(np.setdiff1d(np.arange(len(edges)), sampled[:m]))[: S - m]
    elif kind == "iter200":
        pos = _iter200(D).copy()
    elif kind == "far_query":      # a few vertices 1000 sigma out along an axis: their edges' midpoints have at most 7
        far = rng.permutation(n)[:6]   # others within six grid rings (fewer than K + 1) -> grid_tau_fallback_kernel
        for i, v in enumerate(far):
            pos[v, i % D] = np.float32(1000.0 * (i + 1) * (1 if i % 2 == 0 else -1))
        bad = np.nonzero(np.isin(edges, far).any(axis=1))[0]
        sampled[: len(bad)] = bad
        sampled[len(bad):] = rng.permutation(np.setdiff1d(np.arange(len(edges)), bad))[: S - len(bad)]
    elif kind in ("scaled_1e-4", "scaled_1e4"):
        pos *= np.float32(1e-4 if kind == "scaled_1e-4" else 1e4)
    elif kind != "hubs":
        raise ValueError(kind)
    assert len(np.unique(sampled)) == len(sampled)
    return n, edges, pos, sampled


def _run(search, n, D, edges, pos, sampled, k=K, reorder="off", step=True, seed=1):
    """One engine on one state: rows, the counters of the search, the kernels that ran, one step from the state."""
    from graphem_rapids_amd import _native
    eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, k, len(sampled), seed=seed, reorder=reorder, **SEARCHES[search])
    eng.set_positions(pos)
    eng.timing_enable(True)
    rows = eng.knn_midpoints(sampled)
    again = eng.knn_midpoints(sampled)
    eng.sync()
    names = set(eng.timings())
    _, final, ovf = eng.knn_last_counts()
    stepped = None
    if step:
        eng.set_positions(pos)
        eng.step(sampled)
        stepped = eng.get_positions()
    eng.close()
    assert np.array_equal(rows, again), (search, "two calls")
    if search in KERNEL and k + 1 <= 128:
        assert KERNEL[search] in names, (search, sorted(names))
    if search == "scan":
        assert "grid_build" not in names and "ivf_scan" not in names
    return dict(rows=rows, final=final, ovf=ovf, names=names, step=stepped)


# ----------------------------------------------------------------------------------------------------------------------
# 1. degenerate states

ALL_D = (2, 3, 4, 6, 12, 16)       # D <= 3: ivf_scan_kernel; the matrix-pipe form with KB = 1 up to D = 10, KB = 2 above
STATES = [
    ("collapsed", ALL_D), ("lattice", ALL_D), ("flat_axis", (3,)), ("majority", ALL_D), ("iter200", ALL_D),
    ("far_query", ALL_D), ("hubs", ALL_D), ("scaled_1e-4", ALL_D), ("scaled_1e4", ALL_D),
]


@pytest.mark.parametrize("kind,D", [(kind, D) for kind, Ds in STATES for D in Ds])
def test_every_search_gives_the_oracle_rows_on_degenerate_states(kind, D):
    n, edges, pos, sampled = _case(kind, D)
    ref = oracle.knn_midpoints(pos, edges, sampled, K, tiled=True)
    ref_step = oracle.step(pos, edges, sampled, K)
    scan = _run("scan", n, D, edges, pos, sampled)
    assert np.array_equal(scan["rows"], ref), kind
    assert np.abs(scan["step"] - ref_step).max() <= 1e-4
    for search in _searches(D):
        for reorder in ("off", "bfs"):
            if search == "scan" and reorder == "off":
                continue
            got = _run(search, n, D, edges, pos, sampled, reorder=reorder)
            tag = (kind, D, search, reorder)
            assert np.array_equal(got["rows"], ref), tag           # the oracle's ids in its order, ties on the smaller id
            assert np.array_equal(got["rows"], scan["rows"]), tag
            assert np.abs(got["step"] - ref_step).max() <= 1e-4, tag
            # the same rows, so the same forces up to the order of the fp64 column sums (as test_hip_grid_knn)
            assert np.abs(got["step"] - scan["step"]).max() <= 2e-6, tag
            if kind == "far_query" and search == "grid":
                assert got["ovf"].sum() == 0, tag        # the fallback threshold is finite: nothing goes exhaustive


@pytest.mark.parametrize("D", [2, 3])
def test_grid_on_non_finite_positions(D):
    """Vertices at +inf (the nonfinite state of test_hip_query_cells): grid_coord clamps the infinite coordinates into the
    outermost cell; a query with an infinite coordinate gets no finite threshold (every distance from it is inf or NaN),
    grid_scan_kernel marks its list as overflowed and the selection searches it exhaustively, like the scan does."""
    n, edges = N, _edges()
    rng = np.random.default_rng(40 + D)
    pos = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    pos[rng.permutation(n)[:3], 0] = np.inf
    sampled = rng.permutation(len(edges))[:256].astype(np.int32)
    bad = np.nonzero(~np.isfinite(pos[edges].sum(axis=(1, 2))))[0]
    sampled[: len(bad)] = bad
    nonfinite_q = ~np.isfinite(pos[edges[sampled]].sum(axis=(1, 2)))
    out = {s: _run(s, n, D, edges, pos, sampled, step=False) for s in ("scan", "grid")}
    print(f"\ngrid D={D}: non-finite queries {int(nonfinite_q.sum())}, flagged {int(out['grid']['ovf'][nonfinite_q].sum())}, "
          f"other flagged {int(out['grid']['ovf'][~nonfinite_q].sum())}")
    assert np.array_equal(out["grid"]["rows"], out["scan"]["rows"])
    assert nonfinite_q.sum() > 0 and (out["grid"]["ovf"][nonfinite_q] == 1).all()
    # (finite queries: midpoints at inf are beyond every finite threshold)
    finite_rows = out["grid"]["rows"][~nonfinite_q]
    assert np.isin(finite_rows, bad, invert=True).all()


# ----------------------------------------------------------------------------------------------------------------------
# 2. clusters large enough for the capacity branches

CAP_SEARCHES = [("grid", 3), ("ivf_exact", 3), ("ivf_all", 3), ("ivf_exact", 6), ("ivf_all", 6), ("ivf_exact", 12)]


def _cluster_case(D, members, queries, S, point=3.0, seed=4):
    edges = _edges()
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((N, D)).astype(np.float32)
    inside = _cluster(pos, edges, rng.permutation(N)[:members], point)
    q = rng.permutation(inside)[:queries]
    rest = rng.permutation(np.setdiff1d(np.arange(len(edges)), q))[: S - len(q)]
    return edges, pos, np.concatenate([q, rest]).astype(np.int32), inside


@pytest.mark.parametrize("search,D", CAP_SEARCHES)
def test_candidate_lists_of_8k_to_16k_keys(search, D):
    """13400 of 60000 vertices on one point: ~12 000 coincident midpoints, so a query among them has tau = 0 and a
    candidate list of every one of them -- past the 8192 keys of one extraction half, within the 16384 of a list."""
    edges, pos, sampled, inside = _cluster_case(D, 13400, 32, 256)
    ref = oracle.knn_midpoints(pos, edges, sampled, K)
    got = _run(search, N, D, edges, pos, sampled, step=False)
    print(f"\n{search} D={D}: coincident midpoints {len(inside)}, largest final list {int(got['final'].max())}, "
          f"overflowed {int(got['ovf'].sum())}")
    assert np.array_equal(got["rows"], ref)
    assert 8192 < got["final"].max() <= 16384 and got["ovf"].sum() == 0


@pytest.mark.parametrize("search,D", CAP_SEARCHES)
def test_candidate_lists_past_the_cap(search, D):
    """18000 of 60000 vertices on one point: ~21 600 coincident midpoints, more than a list's 16384 keys: those queries
    go to the exhaustive search of the selection kernel and the rows stay exact."""
    edges, pos, sampled, inside = _cluster_case(D, 18000, 32, 256)
    ref = oracle.knn_midpoints(pos, edges, sampled, K)
    got = _run(search, N, D, edges, pos, sampled, step=False)
    print(f"\n{search} D={D}: coincident midpoints {len(inside)}, largest final list {int(got['final'].max())}, "
          f"overflowed {int(got['ovf'].sum())}")
    assert np.array_equal(got["rows"], ref)
    assert got["ovf"].sum() > 0 and got["final"].max() > 16384


@pytest.mark.parametrize("search,D", [("ivf_exact", 3), ("ivf_all", 3), ("ivf_exact", 6), ("ivf_all", 6),
                                      ("ivf_exact", 12), ("ivf_all", 12)])
def test_ivf_buffers_of_a_tile_overflow(search, D):
    """The LDS buffers of ivf_scan_mfma_kernel (D >= 4; KB = 1 at D = 6, KB = 2 at D = 12).  6700 of 60000 vertices on
    one point give ~3 000 coincident midpoints (>= 2048; within one candidate list); at least 600 of the S = 4096 queries
    are among them.  Every such query has tau = 0 and probes the list that holds the cluster, so:
      * that list is probed by >= 600 > GH_SCAN_QGROUP = 256 queries: each of its tiles walks >= 3 query groups and
        runs the flush between groups (qb0 > q0);
      * in one group of 256 cluster queries against a tile of 512 coincident members every one of the 256 * 512 =
        131 072 pairs passes the f16 pre-filter (F <= 0 at distance 0): far more than PENDCAP = 512 pending pairs, so the
        pairs past it are parked on the spot;
      * every parked pair is a hit (d2 = 0 <= tau): 131 072 > HITBUF (512 at D = 6, 256 at D = 12), so hits spill into
        direct candidate appends.
    At D = 3 the list's tiles go through ivf_scan_kernel instead: the same query groups, and 131 072 hits per group
    against its 1024-entry hit buffer (gh_scan_queries spills the rest into direct appends).
    No counter shows these branches; the rows must still be the oracle's."""
    S4 = 4096
    edges, pos, sampled, inside = _cluster_case(D, 6700, 600, S4, seed=6)
    assert 2048 <= len(inside) <= 16384 and np.isin(sampled, inside).sum() >= 600
    ref = oracle.knn_midpoints(pos, edges, sampled, K, tiled=True)
    got = _run(search, N, D, edges, pos, sampled, step=False)
    print(f"\n{search} D={D}: coincident midpoints {len(inside)}, largest final list {int(got['final'].max())}, "
          f"overflowed {int(got['ovf'].sum())}")
    assert np.array_equal(got["rows"], ref)
    assert got["final"].max() >= len(inside) - 1 and got["ovf"].sum() == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. k at the extraction limits

@pytest.mark.parametrize("kind", ["lattice", "iter200"])
@pytest.mark.parametrize("k", [1, 63, 127, 130])
@pytest.mark.parametrize("search,D", [("grid", 3), ("ivf_exact", 3), ("ivf_exact", 6)])
def test_k_at_the_extraction_limits(kind, k, search, D):
    """K = k + 1 = 128 is the largest the register extraction takes (GH_EXTRACT_MAX_K); past it (k = 130) the engine has no
    filtered search at all -- neither the grid nor the inverted file runs -- and every query goes through the sort
    kernel over all edges."""
    n, edges, pos, sampled = _case(kind, D, S=512)
    ref = oracle.knn_midpoints(pos, edges, sampled, k)
    got = _run(search, n, D, edges, pos, sampled, k=k, reorder="bfs", step=False)
    assert np.array_equal(got["rows"], ref)
    if k + 1 > 128:
        assert "grid_build" not in got["names"] and "ivf_scan" not in got["names"]


# ----------------------------------------------------------------------------------------------------------------------
# 4. approximate inverted file

def _d2_rows(pos, edges, sampled, rows):
    mid = ((pos[edges[:, 0]] + pos[edges[:, 1]]) / np.float32(2.0)).astype(np.float64)
    return ((mid[sampled][:, None, :] - mid[rows]) ** 2).sum(-1)


@pytest.mark.parametrize("kind", ["collapsed", "lattice"])
@pytest.mark.parametrize("probes", [1, 4])
@pytest.mark.parametrize("D", [3, 6])
def test_approximate_ivf_rows_on_mostly_empty_lists(kind, probes, D):
    """ivf_probes = 1 and 4 where most lists are empty (centroids coincide): rows need not be exact, but each row holds k
    distinct valid edge ids, ascending in exact distance, its k-th distance never below the exact one, the same twice."""
    from graphem_rapids_amd import _native
    n, edges, pos, sampled = _case(kind, D)
    exact = oracle.knn_midpoints(pos, edges, sampled, K, tiled=True)
    eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, K, S, knn_method="ivf", ivf_probes=probes)
    assert eng.knn_ivf_config()[1] == probes
    eng.set_positions(pos)
    rows = eng.knn_midpoints(sampled)
    again = eng.knn_midpoints(sampled)
    sizes = eng.knn_ivf_list_sizes()
    eng.close()
    print(f"\nivf probes={probes} {kind} D={D}: empty lists {int((sizes == 0).sum())} of {len(sizes)}, "
          f"rows that differ from exact {int((rows != exact).any(axis=1).sum())} of {S}")
    assert np.array_equal(rows, again)
    assert ((rows >= 0) & (rows < len(edges))).all()
    assert all(len(set(r)) == K for r in rows)
    d = _d2_rows(pos, edges, sampled, rows)
    d_ex = _d2_rows(pos, edges, sampled, exact)
    assert (np.diff(d, axis=1) >= -1e-6 * np.maximum(d[:, 1:], 1e-30)).all()      # ascending (fp32 keys, fp64 here)
    assert (d >= d_ex * (1 - 1e-6)).all()                                          # never better than exact, column by column


# ----------------------------------------------------------------------------------------------------------------------
# 5. set-up inside the normalise launch, invalidated by caller ids

@pytest.mark.parametrize("search", ["grid", "ivf_exact"])
def test_presetup_is_invalidated_when_host_ids_overwrite_the_sample(monkeypatch, search):
    """test_hip_reference_fullsize's test of the same name under the grid and the exact inverted file: run(2) leaves
    the next iteration's set-up (grid_frame_kernel resets the touched-list counter there) done inside its last normalise
    launch, a per-phase call with caller ids overwrites the sample, and the following run must redo the set-up: bit for
    bit the result of an engine that never sets up early."""
    import graphem_rapids_amd as gra
    from graphem_rapids_amd import _native
    n, D, k, S_ = 30000, 3, 10, 256
    edges = gra.random_regular_edges(n, 8, seed=5).astype(np.int32)
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((n, D)).astype(np.float32)
    ids = rng.permutation(len(edges))[:S_].astype(np.int32)

    def sequence():
        eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, k, S_, seed=3, **SEARCHES[search])
        eng.set_positions(pos)
        eng.timing_enable(True)
        eng.run(2)
        cur = eng.get_positions()
        knn = oracle.knn_midpoints(cur, edges, ids, k)
        Fi = eng.intersection_forces(ids, knn)
        eng.run(2)
        out = eng.get_positions()
        eng.sync()
        assert KERNEL[search] in eng.timings()
        eng.close()
        return Fi, out
    Fi_a, out_a = sequence()
    monkeypatch.setenv("GRAPHEM_HIP_NO_PRESETUP", "1")
    Fi_b, out_b = sequence()
    assert np.array_equal(Fi_a, Fi_b)
    assert np.array_equal(out_a, out_b)


# ----------------------------------------------------------------------------------------------------------------------
# 6. runs

def test_device_sampled_runs_agree_across_searches():
    """Ten device-sampled iterations from the 200-iteration layout, one seed: the same samples, exact rows each way."""
    from graphem_rapids_amd import _native
    D = 3
    pos = _iter200(D)
    out = {}
    for search in ("scan", "grid", "ivf_exact"):
        eng = _native.Engine(N, D, _edges(), 1.0, 0.2, 0.5, K, S, seed=17, **SEARCHES[search])
        eng.set_positions(pos)
        eng.timing_enable(True)
        eng.run(10)
        eng.sync()
        out[search] = eng.get_positions()
        if search in KERNEL:
            assert KERNEL[search] in eng.timings()
        eng.close()
    assert np.isfinite(out["scan"]).all()
    assert np.abs(out["grid"] - out["scan"]).max() <= 1e-4
    assert np.abs(out["ivf_exact"] - out["scan"]).max() <= 1e-4


def test_public_auto_choice_takes_the_exact_index():
    """create_graphem(sample_size=4096, knn_method='auto') on 280 000 edges takes the exact inverted file; five iterations
    equal the scan's with the same seed.  The scan side pins knn_distance='exact': with the torch sampler, 'auto' on the
    scan resolves to the cdist parity mode, which ranks differently."""
    import graphem_rapids_amd as gra
    n, D = 70000, 3
    edges = np.ascontiguousarray(gra.random_regular_edges(n, 8, seed=2), dtype=np.int32)
    assert len(edges) >= 262144
    adj = gra.edges_to_adjacency(n, edges)
    out = {}
    for method, dist in (("auto", "auto"), ("scan", "exact")):
        emb = gra.create_graphem(adj, n_components=D, backend="hip", verbose=False, seed=0, init="random",
                                 sample_size=4096, knn_method=method, knn_distance=dist)
        emb._engine.timing_enable(True)   # pylint: disable=protected-access
        out[method] = np.asarray(emb.run_layout(5))
        emb._engine.sync()                # pylint: disable=protected-access
        names = set(emb._engine.timings())   # pylint: disable=protected-access
        if method == "auto":
            assert "ivf_scan" in names, sorted(names)
            assert emb._engine.knn_ivf_config() == (256, 256)   # pylint: disable=protected-access
        else:
            assert "ivf_scan" not in names and "grid_build" not in names
        del emb
    assert np.isfinite(out["auto"]).all()
    assert np.abs(out["auto"] - out["scan"]).max() <= 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# 7. one partitioned case

def test_grid_on_row_partitions_of_a_collapsed_state():
    """The collapsed state on three loopback row partitions with knn_method='grid' (each rank builds its grid from its
    own edges, where tens of thousands of midpoints share one cell): bit-identical ranks, within 2e-6 of the single scan
    engine (test_hip_grid_knn.test_grid_knn_on_row_partitions_and_auto_choice)."""
    import threading
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import partition_rows
    D, world = 3, 3
    n, edges, pos, _ = _case("collapsed", D)
    rng = np.random.default_rng(9)
    stream = np.stack([rng.permutation(len(edges))[:S] for _ in range(3)]).astype(np.int32)
    single = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, K, S, seed=4, knn_method="scan")
    single.set_positions(pos)
    single.run(3, stream)
    ref = single.get_positions()
    single.close()
    lib = _native.load()
    group = lib.gh_loopback_group_create(world)
    engines = []
    for r in range(world):
        chunk, lo, hi = partition_rows(n, world, r)
        e = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, K, S, seed=4, partition=(lo, hi, 0, 0, _native.EDGES_HASHED),
                           knn_method="grid")
        e.gather_layout(world, r, chunk)
        e.comm_init_loopback(group, r)
        e.set_positions(pos)
        engines.append(e)
    errors = []

    def work(e):
        try:
            e.timing_enable(True)
            e.run_partitioned(3, stream)
            e.sync()
        except Exception as exc:  # pylint: disable=broad-exception-caught
            errors.append(exc)
    threads = [threading.Thread(target=work, args=(e,)) for e in engines]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    outs = [e.get_positions() for e in engines]
    assert all("grid_build" in e.timings() for e in engines)
    for e in engines:
        e.comm_destroy()
        e.close()
    lib.gh_loopback_group_destroy(group)
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    assert np.abs(outs[0] - ref).max() <= 2e-6
