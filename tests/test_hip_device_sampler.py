"""The float32 engine's own sample draws, pinned to the documented permutation (gh_sample_id, csrc/common.h) as
tests/sampler_reference.py restates it.

The central assertion: an engine that draws its own ids for iterations t0 .. t0 + T - 1 ends with the same position BITS
as a second engine, same arguments and same start, that runs the same iterations on sampler_reference.stream(E, S, seed,
t0, T) passed as its ids.  After the set-up both runs take the same kernels and ties break on the edge id, so the bar is
tobytes() equality.  Whichever site draws the ids -- knn_setup_kernel in mode 1, the rows staged beside stats_fix, the
set-up folded into the normalise launch -- depends on the step plan, so every route of the plan is run at the smallest
graph that takes it, and each test asserts its route through the phase timers.

(No direct probe of the ids: gh_knn_midpoints refuses a missing id array when sample_size < E.)

The one route that is not bit-identical is the float64 engine: its intersection phase adds with double atomics in no fixed
order (test_hip_f64_phases: two engines stepping the same state agree within 1e-12, a run of three iterations within 1e-9 of
the extended-precision reference).  Its own draws are held to that 1e-9 against the restated stream, and the stream of the
next iteration must miss it by more than 1e-6.

The counter's rule (api.hip step_finish, run_iterations, gh_run_torch_sampled): the iteration number that keys a draw counts
every iteration done since creation, whoever supplied its ids; set_positions does not reset it and the phase probes do not
advance it.

What the file was seen to catch, each on a library built with that one change: the key without `iter` (every test but
test_all_edges_sampled, test_seeds_differ and the `auto` ones); `<=` for `<` in the bit count (test_edge_count_a_power_of_two_and_one_above[0] alone, in the whole
suite); `h->iter` for `h->iter + 1` in the set-up the normalise launch does ahead (every route that sets up ahead).

Needs a real MI355X (`pytest -m gpu`)."""
import functools

import numpy as np
import pytest

import sampler_reference as sr

pytestmark = pytest.mark.gpu

K = 10
PARAMS = (1.0, 0.2, 0.5)   # L_min, k_attr, k_inter
SEEDS = (0, 1, 12345, 1 << 32, (1 << 63) + 5, (1 << 64) - 1)

FUSED = ("spring_scan", "knn_select_intersect", "stats_fix", "normalise")
BLOCK = ("spring*", "knn_setup", "knn_block_select", "integrate")


@functools.lru_cache(maxsize=None)
def _edges(n, extra=0):
    """Random regular of degree 8, sorted by first endpoint; extra: that many more edges (not in the graph) merged in."""
    import graphem_rapids_amd as gra
    edges = np.sort(gra.random_regular_edges(n, 8, seed=n).astype(np.int64), axis=1)
    if extra:
        have = set(map(tuple, edges.tolist()))
        more = [(u, v) for u, v in ((i, i + n // 2) for i in range(n // 2)) if (u, v) not in have][:extra]
        edges = np.concatenate([edges, np.array(more, dtype=np.int64)])
    edges = np.unique(edges, axis=0)
    assert len(edges) == 4 * n + extra
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    edges.setflags(write=False)
    return edges


@functools.lru_cache(maxsize=None)
def _start(n, D, seed=0):
    pos = (0.1 * np.random.default_rng(100 * D + seed).standard_normal((n, D))).astype(np.float32)
    pos.setflags(write=False)
    return pos


def _engine(n, D, edges, S, seed=0, configure=None, **kw):
    from graphem_rapids_amd import _native
    eng = _native.Engine(n, D, edges, *PARAMS, K, S, seed=seed, **kw)
    if configure:
        configure(eng)
    return eng


def _named(names, want):
    return any(nm.startswith(want[:-1]) if want.endswith("*") else nm == want for nm in names)


def _timed_run(eng, T):
    """run(T) on the engine's own draws with the phase timers on: {name: (ms, launches)}."""
    eng.timing_enable(True)
    eng.timing_reset()
    eng.run(T)
    eng.sync()
    names = eng.timings()
    eng.timing_enable(False)
    return names


def _assert_route(names, expect=(), forbid=()):
    for want in expect:
        assert _named(names, want), (want, sorted(names))
    for bad in forbid:
        assert not _named(names, bad), (bad, sorted(names))


def _own_and_restated(n, D, S, T, edges=None, seed=0, t0=0, **kw):
    """(positions after T own draws, positions after the restated stream, phase names of the own run).  t0 > 0: both engines
    first run t0 iterations on the restated ids 0 .. t0 - 1, so the own draws are those of iterations t0 .. t0 + T - 1."""
    edges = _edges(n) if edges is None else edges
    E = len(edges)
    Seff = min(S, E)
    own, ref = _engine(n, D, edges, S, seed, **kw), _engine(n, D, edges, S, seed, **kw)
    try:
        for eng in (own, ref):
            eng.set_positions(_start(n, D))
            if t0:
                eng.run(t0, sr.stream(E, Seff, seed, 0, t0))
        names = _timed_run(own, T)
        ref.run(T, sr.stream(E, Seff, seed, t0, T))
        return own.get_positions(), ref.get_positions(), names
    finally:
        own.close()
        ref.close()


def _assert_pinned(n, D, S, T=4, expect=(), forbid=(), **kw):
    a, b, names = _own_and_restated(n, D, S, T, **kw)
    _assert_route(names, expect, forbid)
    assert np.isfinite(b).all()
    assert a.tobytes() == b.tobytes(), f"own draws differ from the restated stream: max|diff| {np.abs(a - b).max():.3g}"
    return names


# ---- routes ------------------------------------------------------------------------------------------------------------

def test_block_select():
    """2000 vertices of degree 8, E = 8000 < GH_SCAN_MIN_EDGES: the exhaustive search; knn_setup_kernel draws the ids (mode 1) in every iteration."""
    names = _assert_pinned(2000, 3, 64, expect=BLOCK, forbid=("spring_scan",))
    assert names["knn_setup"][1] == 4, names


@pytest.mark.parametrize("S", [1, 255, 256, 300])
@pytest.mark.parametrize("D", [2, 3])
def test_fused_thresholds_inside_the_launch(D, S):
    """E = 16800: the fused launch computes the thresholds itself; iterations 1 .. 3 are set up inside the normalise launch
    of the iteration before, from rows staged beside stats_fix (one stand-alone set-up, for iteration 0)."""
    names = _assert_pinned(4200, D, S, expect=FUSED, forbid=("knn_tau", "knn_block_select"))
    assert names["knn_setup"][1] == 1 and names["normalise"][1] == 4, names


@pytest.mark.parametrize("extra", [0, 1])
def test_edge_count_a_power_of_two_and_one_above(extra):
    """E = 16384 = 2^14 takes 14 bits, E = 16385 takes 15: the two sizes at which an off-by-one bit count shows, on the
    fused path, whose floor is exactly 2^14."""
    edges = _edges(4096, extra)
    assert len(edges) == 16384 + extra
    _assert_pinned(4096, 3, 256, T=6, edges=edges, expect=FUSED, forbid=("knn_block_select",))


@pytest.mark.parametrize("D", [6, 12, 17])
def test_wide_and_generic_rows(D):
    """Row strides 8 and 16 (the wide pre-filter of the fused kernel) and 20 (D = 17: generic kernels, exhaustive search)."""
    if D <= 16:
        _assert_pinned(4200, D, 256, expect=FUSED, forbid=("knn_block_select",))
    else:
        _assert_pinned(4200, D, 256, expect=("spring*", "knn_setup", "knn_block_select"), forbid=("spring_scan",))


@pytest.mark.parametrize("coarse", ["on", "off"])
def test_query_cell_filter(coarse):
    """The query-cell form of the fused launch, thresholds from the coarse table inside it (on) or from a launch of their
    own (off)."""
    def configure(eng):
        eng.set_scan_filter("cells")
        eng.set_coarse_tau(coarse)
        assert eng.scan_filter() == "cells" and eng.coarse_tau() == (coarse == "on")
    names = _assert_pinned(20000, 3, 256, configure=configure, expect=FUSED,
                           forbid=("knn_tau",) if coarse == "on" else ())
    assert ("knn_tau" in names) == (coarse == "off"), sorted(names)


def test_cdist_distance():
    _assert_pinned(4200, 3, 256, knn_distance="cdist", expect=("spring_scan", "knn_select_cdist*"))


@pytest.mark.parametrize("method,kw,expect", [("grid", {}, ("grid_build",)),
                                              ("ivf", {"ivf_probes": -1}, ("ivf_probe", "ivf_scan"))])
def test_grid_and_exact_inverted_file(method, kw, expect):
    _assert_pinned(4200, 3, 256, knn_method=method, expect=expect, forbid=("spring_scan", "knn_block_select"), **kw)


def test_wave_select():
    """S = 2048: the wave-per-query selection (no column sums ride along)."""
    _assert_pinned(4200, 3, 2048, expect=FUSED, forbid=("knn_block_select",))


def test_all_edges_sampled():
    """S >= E: the engine's own ids are arange(E) (no permutation is drawn), equal to arange(E) given explicitly.  An
    engine with S >= E uses arange whatever it is given, so the explicit ids are also put to the CPU oracle: one step
    within 1e-4, the bar of test_hip_parity's one-step comparisons."""
    import oracle
    n, D = 4200, 3
    edges = _edges(n)
    E = len(edges)
    arange = np.arange(E, dtype=np.int32)
    own, ref = _engine(n, D, edges, E), _engine(n, D, edges, E)
    try:
        own.set_positions(_start(n, D))
        ref.set_positions(_start(n, D))
        own.run(1)
        err = float(np.abs(own.get_positions() - oracle.step(_start(n, D), edges, arange, K, *PARAMS)).max())
        print(f"\nS = E: one step on the engine's own ids against the oracle on arange(E): {err:.3g}")
        assert err <= 1e-4
        own.run(1)
        ref.run(2, np.tile(arange, (2, 1)))
        assert own.get_positions().tobytes() == ref.get_positions().tobytes()
    finally:
        own.close()
        ref.close()


@pytest.mark.parametrize("D,S", [(3, 256), (2, 300)])
def test_standalone_setup_every_iteration(D, S, monkeypatch):
    """GRAPHEM_HIP_NO_PRESETUP=1: knn_setup_kernel draws every iteration's ids itself."""
    monkeypatch.setenv("GRAPHEM_HIP_NO_PRESETUP", "1")
    names = _assert_pinned(4200, D, S, expect=FUSED)
    assert names["knn_setup"][1] == 4, names


@pytest.mark.parametrize("seed", SEEDS)
def test_seeds(seed):
    """All 64 bits of the seed reach the key: 2^32 does not collide with 0, 2^63 + 5 not with 5."""
    _assert_pinned(4200, 3, 256, seed=seed, expect=FUSED)


def test_seeds_differ():
    outs = [_own_and_restated(4200, 3, 256, 2, seed=s)[0].tobytes() for s in (0, 1 << 32, 5, (1 << 63) + 5)]
    assert len(set(outs)) == 4


def test_later_iterations():
    """Own draws that start at iteration 5 (after five given ones) are those of iterations 5 .. 8, not 0 .. 3."""
    a, b, _ = _own_and_restated(4200, 3, 256, 4, t0=5)
    assert a.tobytes() == b.tobytes()


def test_float64_engine_draws_the_same_ids():
    """Both engines against the one restated stream each: the float32 engine to the bit, the float64 engine within 1e-9
    (double atomics in no fixed order: module docstring), and the stream one iteration late misses it by > 1e-6."""
    n, D, S, T = 4200, 3, 256, 3
    edges = _edges(n)
    E = len(edges)
    _assert_pinned(n, D, S, T=T, expect=FUSED)
    start = np.asarray(_start(n, D), dtype=np.float64)
    outs = []
    for ids in (None, sr.stream(E, S, 0, 0, T), sr.stream(E, S, 0, 1, T)):
        eng = _engine(n, D, edges, S, dtype="float64")
        try:
            eng.set_positions(start)
            eng.run(T, ids)
            outs.append(eng.get_positions())
        finally:
            eng.close()
    assert outs[0].dtype == np.float64 and np.isfinite(outs[0]).all()
    err, late = float(np.abs(outs[0] - outs[1]).max()), float(np.abs(outs[0] - outs[2]).max())
    print(f"\nfloat64 own draws against the restated stream: {err:.3e} of bar 1e-9; one iteration late: {late:.3e}")
    assert err <= 1e-9
    assert late > 1e-6


# ---- the counter -------------------------------------------------------------------------------------------------------

def test_counter_counts_every_iteration_whoever_gave_its_ids():
    n, D, S, seed = 4200, 3, 256, 7
    edges = _edges(n)
    E = len(edges)
    rng = np.random.default_rng(11)
    given = rng.permutation(E)[:S].astype(np.int32)
    probe = rng.permutation(E)[:S].astype(np.int32)
    p0, p1 = _start(n, D), _start(n, D, seed=1)
    own = sr.stream(E, S, seed, 0, 7)
    a, b = _engine(n, D, edges, S, seed), _engine(n, D, edges, S, seed)
    try:
        a.set_positions(p0)
        a.run(2)                          # own 0, 1
        a.step(given)                     # iteration 2: given ids
        a.step()                          # own 3
        b.set_positions(p0)
        b.run(4, np.stack([own[0], own[1], given, own[3]]))
        mid_a = a.get_positions()
        assert mid_a.tobytes() == b.get_positions().tobytes()
        # the phase probes neither advance the counter nor leave a stale set-up behind
        knn = a.knn_midpoints(probe)
        assert np.array_equal(knn, b.knn_midpoints(probe))
        a.spring_forces()
        a.intersection_forces(probe, knn)
        assert a.get_positions().tobytes() == mid_a.tobytes()
        a.set_positions(p1)               # does not reset the counter
        a.run(3)                          # own 4, 5, 6
        b.set_positions(p1)
        b.run(3, own[4:7])
        assert a.get_positions().tobytes() == b.get_positions().tobytes()
    finally:
        a.close()
        b.close()


def test_counter_after_a_torch_sampled_run():
    """run_torch_sampled(2, state) then run(2): the own draws are those of iterations 2 and 3."""
    import torch
    from graphem_rapids_amd import _native
    n, D, S, seed = 4200, 3, 256, 3
    edges = _edges(n)
    E = len(edges)
    torch.manual_seed(1234)
    state = torch.get_rng_state().numpy().copy()
    torch_ids = _native.torch_randperm_prefix(state.copy(), E, S, 2)
    a, b = _engine(n, D, edges, S, seed), _engine(n, D, edges, S, seed)
    try:
        a.set_positions(_start(n, D))
        a.run_torch_sampled(2, state)
        a.run(2)
        b.set_positions(_start(n, D))
        b.run(2, torch_ids)
        b.run(2, sr.stream(E, S, seed, 2, 2))
        assert a.get_positions().tobytes() == b.get_positions().tobytes()
    finally:
        a.close()
        b.close()


# ---- partitions --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("finish", ["own", "gathered", "overlap"])
@pytest.mark.parametrize("world,n", [(2, 4200), (3, 4200), (2, 20000)])   # 20000: every rank searches >= GH_SCAN_MIN_EDGES edges
def test_partitioned_ranks_draw_the_restated_ids(world, n, finish):
    """Every rank draws for itself (step_in_process without ids): all ranks end with identical bits, within the 2e-6 of
    test_hip_parity.test_partitioned_engines_equal_single_engine of one engine run on the restated ids."""
    import torch
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import HipShardEngine, partition_rows, step_in_process
    D, S, T, seed = 3, 256, 3, 12345
    edges = _edges(n)
    E = len(edges)
    single = _engine(n, D, edges, S, seed)
    try:
        single.set_positions(_start(n, D))
        single.run(T, sr.stream(E, S, seed, 0, T))
        ref = single.get_positions()
    finally:
        single.close()
    shards = []
    for r in range(world):
        chunk, lo, hi = partition_rows(n, world, r)
        sh = HipShardEngine(n, D, edges, *PARAMS, K, S, seed, (lo, hi, 0, 0, _native.EDGES_HASHED), 0)
        if finish == "own":
            sh.rank_layout(world, r, chunk, packed=True)
        elif finish == "overlap":
            sh.overlap_layout(world, r, chunk)
        else:
            sh.gather_layout(world, r, chunk)
        sh.set_positions(_start(n, D))
        shards.append(sh)
    for _ in range(T):
        step_in_process(shards, finish, None)
    torch.cuda.synchronize()
    outs = [sh.get_positions() for sh in shards]
    for got in outs:
        assert got.tobytes() == outs[0].tobytes()
    err = float(np.abs(outs[0] - ref).max())
    print(f"\nworld={world} n={n} {finish}: max|diff| against one engine on the restated ids {err:.3g}")
    assert err <= 2e-6


# ---- the public class --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 12345])
def test_public_class_passes_its_seed_as_the_key(seed):
    """GraphEmbedderHIP(seed=s, sampler='device') keys the device sampler with s itself (embedder_hip.py): run_layout(3)
    equals an engine with seed=s on the restated stream, from the start the class draws (np.random.seed(s); randn * 0.1)."""
    import graphem_rapids_amd as gra
    n, D, S = 4200, 3, 256
    adj = gra.edges_to_adjacency(n, _edges(n))
    emb = gra.GraphEmbedderHIP(adj, n_components=D, sample_size=S, n_neighbors=K, sampler="device", seed=seed,
                               init="random", verbose=False)
    assert emb.sampler == "device" and emb._engine_seed == seed
    got = emb.run_layout(3)
    edges = emb._edges_np
    E = len(edges)
    np.random.seed(seed)
    p0 = np.random.randn(n, D) * 0.1
    eng = _engine(n, D, edges, S, seed)
    try:
        eng.set_positions(p0)
        eng.run(3, sr.stream(E, S, seed, 0, 3))
        assert got.tobytes() == eng.get_positions().tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("n,want", [(262144, "torch"), (262146, "device")])
def test_auto_sampler_turns_to_the_device_above_2_20_edges(n, want):
    import graphem_rapids_amd as gra
    edges = gra.random_regular_edges(n, 8, seed=1)
    assert len(edges) == 4 * n and (len(edges) <= (1 << 20)) == (want == "torch")
    emb = gra.GraphEmbedderHIP(gra.edges_to_adjacency(n, edges), n_components=3, sampler="auto", seed=0, init="random",
                               verbose=False)
    assert emb.n_edges == 4 * n and emb.sampler == want
    emb.run_layout(1)
    assert np.isfinite(emb.positions).all()
