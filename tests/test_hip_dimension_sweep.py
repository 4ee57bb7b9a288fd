"""Every launch site that picks a kernel by embedding dimension, at every dimension: D = 2..16 take the instantiation
csrc/dispatch.h hands out (one wrong (D, LD) pair at one site is what this file is for), D = 17 the generic kernels at a
row stride of 20.  The graphs are the smallest that still take each path:

  fused     random regular, 4200 vertices of degree 8 = 16 800 edges (GH_SCAN_MIN_EDGES is 16384): the fused spring+scan
            kernels and knn_select with the intersection phase
  unfused   2000 vertices of degree 8: spring_kernel / the generic kernel, knn_block_select, integrate_kernel
  cdist     the 4200-vertex graph with knn_distance="cdist": knn_select_cdist_kernel and the fused replay
  ivf       the 4200-vertex graph with knn_method="ivf", ivf_probes=-1 (the exact inverted file)
  hub300    3000 vertices of degree 8 and one hub of degree ~300: long rows in one launch (long_rows_kernel)
  hub1100   the same with a hub of degree ~1100 (above GH_LONG_ONE_LAUNCH_MAX_DEG): long_terms_kernel + long_sum_kernel
  two ranks two row partitions through distributed.step_in_process: the dimensioned knn_merge_kernel

Expected values are the CPU oracle's with the bars of test_hip_parity.test_random_graphs_against_oracle (spring forces
bit-identical, KNN ids identical, intersection forces rtol 1e-6, one step <= 1e-4), ATen's rows as in test_hip_cdist, and
two ranks against one engine <= 2e-6 as in test_hip_parity.  Needs a real MI355X (`pytest -m gpu`)."""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

DIMS = list(range(2, 18))
K, S = 10, 64
PARAMS = (1.0, 0.2, 0.5)   # L_min, k_attr, k_inter


@functools.lru_cache(maxsize=None)
def _edges(n, hub_degree=0):
    import graphem_rapids_amd as gra
    edges = gra.random_regular_edges(n, 8, seed=n).astype(np.int64)
    if hub_degree:
        hub = 7
        nb = np.random.default_rng(hub_degree).choice(n, size=hub_degree, replace=False)
        nb = nb[nb != hub]
        extra = np.stack([np.minimum(hub, nb), np.maximum(hub, nb)], axis=1)
        edges = np.unique(np.concatenate([np.sort(edges, axis=1), extra]), axis=0)
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    edges.setflags(write=False)
    return edges


@functools.lru_cache(maxsize=None)
def _case(n, D, hub_degree=0):
    """Edges, positions, sampled ids and the oracle's answers for them: computed once, shared, read-only."""
    edges = _edges(n, hub_degree)
    rng = np.random.default_rng(1000 * D + n + hub_degree)
    pos = rng.standard_normal((n, D)).astype(np.float32)
    sampled = rng.permutation(len(edges))[:S].astype(np.int32)
    case = dict(n=n, D=D, edges=edges, pos=pos, sampled=sampled,
                spring=oracle.spring_forces(pos, edges, PARAMS[0], PARAMS[1]),
                knn=oracle.knn_midpoints(pos, edges, sampled, K),
                step=oracle.step(pos, edges, sampled, K, *PARAMS))
    case["inter"] = oracle.intersection_forces(pos, edges, sampled, case["knn"], PARAMS[2])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _timed_step(eng, sampled, expect, D):
    """One step with the phase timers on; for D <= 16 the step must have gone through the phases named in `expect`
    (a name ending in * stands for every name it begins)."""
    eng.timing_enable(True)
    eng.timing_reset()
    eng.step(sampled)
    names = sorted(eng.timings())
    eng.timing_enable(False)
    if D <= 16:
        for want in expect:
            assert any(nm.startswith(want[:-1]) if want.endswith("*") else nm == want for nm in names), (want, names)
    return names


def _check_against_oracle(c, expect, **kw):
    from graphem_rapids_amd import _native
    eng = _native.Engine(c["n"], c["D"], c["edges"], *PARAMS, K, S, **kw)
    try:
        eng.set_positions(c["pos"])
        assert np.array_equal(eng.spring_forces(), c["spring"])
        assert np.array_equal(eng.knn_midpoints(c["sampled"]), c["knn"])
        Fi = eng.intersection_forces(c["sampled"], c["knn"])
        np.testing.assert_allclose(Fi, c["inter"], rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(c["inter"]).max())))
        names = _timed_step(eng, c["sampled"], expect, c["D"])
        err = float(np.abs(eng.get_positions() - c["step"]).max())
        print(f"D={c['D']} n={c['n']} {kw}: one step max|diff| {err:.3g}; phases {' '.join(names)}")
        assert err <= 1e-4
    finally:
        eng.close()


@pytest.mark.parametrize("D", DIMS)
def test_fused_step(D):
    _check_against_oracle(_case(4200, D), ("spring_scan", "knn_select_intersect", "stats_fix"))


@pytest.mark.parametrize("D", DIMS)
def test_unfused_step(D):
    _check_against_oracle(_case(2000, D), ("spring*", "knn_block_select", "integrate"))


@pytest.mark.parametrize("D", DIMS)
def test_exact_inverted_file(D):
    _check_against_oracle(_case(4200, D), ("ivf_probe", "ivf_scan"), knn_method="ivf", ivf_probes=-1)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("hub_degree", [300, 1100])
def test_hub_rows(D, hub_degree):
    _check_against_oracle(_case(3000, D, hub_degree), ("spring_long",))


@pytest.mark.parametrize("D", DIMS)
def test_cdist_rows_and_step(D):
    """knn_distance="cdist": ATen's rows (oracle/aten_cdist_topk.cpp) and one step of the oracle in its ATen mode."""
    from graphem_rapids_amd import _native
    c = _case(4200, D)
    eng = _native.Engine(c["n"], D, c["edges"], *PARAMS, K, S, knn_distance="cdist")
    try:
        eng.set_positions(c["pos"])
        knn = eng.knn_midpoints(c["sampled"])
        _, unresolved = eng.knn_cdist_stats()
        assert np.array_equal(knn, oracle.knn_midpoints_aten(c["pos"], c["edges"], c["sampled"], K))
        assert unresolved == 0
        names = _timed_step(eng, c["sampled"], ("knn_select_cdist*", "cdist_replay*"), D)
        err = float(np.abs(eng.get_positions() - oracle.step_aten(c["pos"], c["edges"], c["sampled"], K)).max())
        print(f"D={D} cdist: one step max|diff| {err:.3g}; phases {' '.join(names)}")
        assert err <= 1e-4
    finally:
        eng.close()


@pytest.mark.parametrize("D", DIMS)
def test_two_ranks_equal_one_engine(D):
    import torch
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import HipShardEngine, partition_rows, step_in_process
    c = _case(4200, D)
    n, world = c["n"], 2
    single = _native.Engine(n, D, c["edges"], *PARAMS, K, S)
    single.set_positions(c["pos"])
    single.step(c["sampled"])
    ref = single.get_positions()
    single.close()
    shards = []
    for r in range(world):
        chunk, lo, hi = partition_rows(n, world, r)
        shards.append(HipShardEngine(n, D, c["edges"], *PARAMS, K, S, 0, (lo, hi, 0, 0, _native.EDGES_HASHED), 0))
        shards[-1].rank_layout(world, r, chunk, packed=True)
        shards[-1].set_positions(c["pos"])
    shards[0].eng.timing_enable(True)
    shards[0].eng.timing_reset()
    step_in_process(shards, "own", c["sampled"])
    torch.cuda.synchronize()
    names = sorted(shards[0].eng.timings())
    assert "knn_merge_intersect" in names, names
    outs = [sh.get_positions() for sh in shards]
    err = float(np.abs(outs[0] - ref).max())
    print(f"D={D} two ranks: max|diff| against one engine {err:.3g}")
    assert err <= 2e-6
    assert np.array_equal(outs[0], outs[1])
