"""The float64 engine (csrc/f64.hip) phase by phase against tests/f64_reference.py -- one iteration of the reference in
extended precision (anchored on the reference's own float64 output by tests/test_f64_reference_cpu.py) -- at the shapes its
kernels branch on.  Which row of code each test names:

  f64_spring4_kernel<2>, <3>, <4>; f64_spring_kernel (D = 1, 5..32)   test_spring_forces_on_a_degree_ladder, _on_hard_clouds
  degree 0..5, 7, 8, 9, 12, 1000, 5000; unsorted, swapped edge list   the same (f64_reference.degree_ladder)
  D = 33 refused                                                      test_more_than_32_components_are_refused
  f64_intersect_kernel, `< 0`, i > j, shared vertices, atomics        test_intersection_forces_on_planted_pairs
  f64_mid4_kernel<2>, <3>, <4>, f64_mid_kernel                        test_runs_with_the_device_sampler (D = 3), the filtered
                                                                      search of tests/test_hip_f64.py (D = 1..16), _one_million
  f64_sum / f64_centre / f64_scale, f64_block_columns, nblocks        test_update_kernels_alone, test_three_updates_in_a_row
  a step on the filtered search                                       tests/test_hip_f64.py (strengthened), _one_million (slow)
  f64_sample_kernel + gh_sample_id                                    test_runs_with_the_device_sampler
  gh_f64_set_positions_f32 / gh_f64_get_positions_f32                 test_float32_accessors_of_a_float64_handle

Bars (tests/test_hip_f64.py's): spring forces 1e-13 and intersection forces 1e-12 relative to max(1, max|ref|); positions after
one step 1e-10, after three 1e-9, times max(1, max|input coordinate|) where the input is shifted or scaled.  Every test prints
what it measured.  Needs a real MI355X."""
import numpy as np
import pytest

import f64_reference as reference

pytestmark = pytest.mark.gpu

PRM = (1.0, 0.2, 0.5)     # L_min, k_attr, k_inter


def _rel(a, ref):
    ref = np.asarray(ref, dtype=reference.LD)
    return float(np.abs(np.asarray(a, dtype=reference.LD) - ref).max() / max(1.0, float(np.abs(ref).max())))


def _abs(a, ref):
    return float(np.abs(np.asarray(a, dtype=reference.LD) - ref).max())


def _engine(n, D, edges, k=10, S=0, seed=0):
    from graphem_rapids_amd import _native
    return _native.Engine(n, D, edges, *PRM, k, S, seed=seed, dtype="float64")


def _spring_case(D, pos, n, edges):
    eng = _engine(n, D, edges)
    try:
        eng.set_positions(pos)
        F = eng.spring_forces()
    finally:
        eng.close()
    assert F.dtype == np.float64 and F.shape == (n, D)
    ref = reference.spring_forces(pos, edges, PRM[0], PRM[1])
    deg = np.bincount(edges.ravel(), minlength=n)
    assert not F[deg == 0].any()                                     # an isolated vertex feels nothing, exactly
    return _rel(F, ref), float(np.abs(ref).max())


@pytest.mark.parametrize("D", range(1, 33))
def test_spring_forces_on_a_degree_ladder(D):
    """Every instantiation of the spring kernels (spring4<2>, <3>, <4>; the general kernel at D = 1 -- its four-at-a-time
    branch -- and 5..32 = F64_MAXD) on degrees 0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 1000 and 5000 (groups of four and every tail),
    the edge list shuffled and its endpoints swapped."""
    n, edges = reference.degree_ladder()
    pos = np.random.default_rng(100 + D).standard_normal((n, D))
    err, mx = _spring_case(D, pos, n, edges)
    print(f"\nspring ladder D={D}: {err:.3e} of bar 1e-13 (max|ref| {mx:.3g})")
    assert err <= 1e-13


@pytest.mark.parametrize("kind", ["collapsed", "huge", "coincident"])
@pytest.mark.parametrize("D", [2, 3, 4, 7])
def test_spring_forces_on_hard_clouds(D, kind):
    """The ladder on a cloud of 1e-9 around 5.0, on one scaled by 1e6, and with 100 edges of length exactly 0 (the
    reference's diff / (0 + 1e-6) is 0, not NaN)."""
    n, edges = reference.degree_ladder()
    pos = np.random.default_rng(200 + D).standard_normal((n, D))
    if kind == "collapsed":
        pos = pos * 1e-9 + 5.0
    elif kind == "huge":
        pos = pos * 1e6
    else:
        used, pick = set(), []
        for e in np.random.default_rng(7).permutation(len(edges)):      # 100 edges with no vertex in common
            u, v = (int(x) for x in edges[e])
            if len(pick) < 100 and u not in used and v not in used:
                used.update((u, v))
                pick.append(e)
        pos[edges[pick, 1]] = pos[edges[pick, 0]]
        assert (pos[edges[:, 0]] == pos[edges[:, 1]]).all(axis=1).sum() >= 100
    err, mx = _spring_case(D, pos, n, edges)
    print(f"\nspring {kind} D={D}: {err:.3e} of bar 1e-13 (max|ref| {mx:.3g})")
    assert err <= 1e-13


def test_more_than_32_components_are_refused():
    n, edges = 64, np.stack([np.arange(63), np.arange(1, 64)], axis=1).astype(np.int32)
    with pytest.raises(ValueError, match="up to 32 components"):
        _engine(n, 33, edges)
    _engine(n, 32, edges).close()


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 8, 16, 31, 32])
def test_intersection_forces_on_planted_pairs(D):
    """f64_intersect_kernel on pairs planted by f64_reference.planted_intersections: 886 listed crossings (a pair listed
    twice counts twice), 912 pairs with i > j, 30 that touch, 30 collinear overlapping ones and 30 sharing a vertex -- none of
    which may push -- and one vertex that 256 crossing pairs add to.  Coordinates 0 and 1 are small integers, so the
    reference's decision is the truth.  D = 1: zeros on both sides."""
    pos, edges, sampled, knn, hub = reference.planted_intersections(D)
    ref = reference.intersection_forces(pos, edges, sampled, knn, PRM[2])
    if D >= 2:       # the condition on the input, on the reference alone
        counts = reference.classify_planted(pos, edges, sampled, knn, hub)
        assert 4 * counts["crossing"] >= counts["listed"] and counts["hub"] >= 200
        assert min(counts["touching"], counts["collinear"], counts["shared"], counts["i_gt_j"]) >= 1
        assert len(reference.crossing_pairs(pos, edges, sampled, knn)[0]) == counts["crossing"]
    else:
        assert not ref.any()
    eng = _engine(len(pos), D, edges, k=reference.PLANTED_K, S=len(sampled))
    try:
        eng.set_positions(pos)
        F = eng.intersection_forces(sampled, knn)
        again = eng.intersection_forces(sampled, knn)
    finally:
        eng.close()
    err = _rel(F, ref)
    print(f"\nintersection planted D={D}: {err:.3e} of bar 1e-12 (max|ref| {float(np.abs(ref).max()):.3g}, hub {np.abs(F[hub]).max():.3g})")
    assert err <= 1e-12 and _rel(again, ref) <= 1e-12
    assert np.array_equal(F.any(axis=1), np.asarray(ref != 0).any(axis=1))     # exactly the vertices of crossing pairs are pushed
    if D == 1:
        assert not F.any()


def _regular_or_path(n, seed):
    import graphem_rapids_amd as gra
    if n < 6:
        return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)
    return np.ascontiguousarray(gra.random_regular_edges(n, 4, seed=seed), dtype=np.int32)


def _shifted_start(n, D, seed):
    pos = np.random.default_rng(seed).standard_normal((n, D))
    pos[:, 0] += 1000.0
    return pos


UPDATE_SHAPES = [(2, 7), (3, 5), (257, 31), (174763, 3), (174762, 3), (1000003, 1), (1000003, 2), (1000003, 3), (400001, 5),
                 (300007, 6), (300007, 7), (150001, 12), (100003, 16), (60013, 31), (60013, 32)]


@pytest.mark.parametrize("n,D", UPDATE_SHAPES)
def test_update_kernels_alone(n, D):
    """sample_size = 0: a step is spring forces + f64_sum / f64_centre / f64_scale.  Shapes on both sides of 2048 * 256
    elements (the cap on the workgroups: beyond it the grid-stride loops take further trips), D with D / gcd(256, D) = 1, 3,
    5, 7, 31 (the multiple the workgroup count is rounded to; f64_block_columns' column of a thread) and fewer elements than
    one such multiple of workgroups holds (n = 2, D = 7).  Start shifted by +1000 in column 0: centring has to cancel it."""
    edges = _regular_or_path(n, D)
    pos = _shifted_start(n, D, 300 + D)
    eng = _engine(n, D, edges)
    try:
        eng.set_positions(pos)
        eng.step()
        out = eng.get_positions()
    finally:
        eng.close()
    ref = reference.step(pos, edges, None, None, *PRM)
    bar = 1e-10 * max(1.0, float(np.abs(pos).max()))
    err = _abs(out, ref)
    print(f"\nupdate n={n} D={D}: {err:.3e} of bar {bar:.3e}")
    assert err <= bar
    if n >= 257:
        assert np.abs(out.mean(axis=0)).max() <= 1e-9 and np.abs(out.std(axis=0, ddof=1) - 1.0).max() <= 1e-5


def test_three_updates_in_a_row():
    n, D = 1000003, 3
    edges = _regular_or_path(n, D)
    pos = _shifted_start(n, D, 303)
    eng = _engine(n, D, edges)
    try:
        eng.set_positions(pos)
        for _ in range(3):
            eng.step()
        out = eng.get_positions()
    finally:
        eng.close()
    ref = pos
    for _ in range(3):
        ref = reference.step(ref, edges, None, None, *PRM)
    bar = 1e-9 * max(1.0, float(np.abs(pos).max()))
    err = _abs(out, ref)
    print(f"\nthree updates n={n} D={D}: {err:.3e} of bar {bar:.3e}")
    assert err <= bar


def _gapped_start(n, D, edges, k, S, seed, iters):
    """A Gaussian start whose reference trajectory under sample_ids(E, S, seed, t) has neighbour rows that do not hinge on
    the last bits of a distance (knn_gap >= 1e-9 on every iteration): decided on the reference alone.  Returns the start,
    the sampled ids and rows of every iteration and the final positions."""
    E = len(edges)
    for start_seed in range(8):
        pos0 = np.random.default_rng(1000 * seed + start_seed).standard_normal((n, D))
        pos, trace, ok = pos0, [], True
        for t in range(iters):
            ids = reference.sample_ids(E, S, seed, t)
            p64 = np.asarray(pos, dtype=np.float64)
            mid = np.asarray(reference.midpoints(p64, edges), dtype=np.float64)
            if reference.knn_gap(mid, ids, k) < 1e-9:
                ok = False
                break
            knn = reference.knn_rows(mid, ids, k)
            trace.append((ids, knn))
            pos = reference.step(p64, edges, ids, knn, *PRM)
        if ok:
            return pos0, trace, pos
    raise AssertionError("no start with well separated neighbour rows among 8 seeds")


@pytest.mark.parametrize("seed", [0, 12345])
@pytest.mark.parametrize("n", [5000, 40000])
def test_runs_with_the_device_sampler(n, seed):
    """eng.run(3) without a sample stream: f64_sample_kernel draws gh_sample_id(E, seed, t, .) for t = 0, 1, 2.  Against the
    reference iterated with f64_reference.sample_ids and its own brute-force rows; 20000 edges take the full passes, 160000
    the filtered search.  (The reference restarts every iteration from its positions rounded to double, as the engine
    stores them.)"""
    import graphem_rapids_amd as gra
    D, k, S = 3, 10, 64
    edges = np.ascontiguousarray(gra.random_regular_edges(n, 8, seed=1), dtype=np.int32)
    assert (len(edges) >= 131072) == (n == 40000)
    pos0, trace, ref = _gapped_start(n, D, edges, k, S, seed, 3)
    eng = _engine(n, D, edges, k=k, S=S, seed=seed)
    try:
        eng.set_positions(pos0)
        assert np.array_equal(eng.knn_midpoints(trace[0][0]), trace[0][1])
        eng.run(3)
        out = eng.get_positions()
    finally:
        eng.close()
    err = _abs(out, ref)
    print(f"\nrun(3) device sampler n={n} seed={seed}: {err:.3e} of bar 1e-9")
    assert err <= 1e-9
    other = reference.sample_ids(len(edges), S, seed + 1, 0)
    assert not np.array_equal(other, trace[0][0])


def test_sample_size_of_all_edges_uses_arange_and_too_many_neighbours_raise():
    """S >= E: every edge is a query, in order (pt.py:412), whatever ids are passed; k + 1 > E raises RuntimeError as on the
    float32 engine; two engines stepping the same state agree within 1e-12 (the order of the double atomics)."""
    import graphem_rapids_amd as gra
    n, D, k = 300, 3, 10
    edges = np.ascontiguousarray(gra.random_regular_edges(n, 4, seed=3), dtype=np.int32)
    E = len(edges)
    pos = np.random.default_rng(9).standard_normal((n, D))
    mid = np.asarray(reference.midpoints(pos, edges), dtype=np.float64)
    ids = np.arange(E, dtype=np.int32)
    assert reference.knn_gap(mid, ids, k) >= 1e-9
    knn = reference.knn_rows(mid, ids, k)
    ref = reference.step(pos, edges, ids, knn, *PRM)
    outs = []
    for S in (E, E + 1000):
        eng = _engine(n, D, edges, k=k, S=S)
        try:
            eng.set_positions(pos)
            assert np.array_equal(eng.knn_midpoints(), knn)
            eng.run(1)
            outs.append(eng.get_positions())
        finally:
            eng.close()
    errs = [_abs(o, ref) for o in outs]
    print(f"\nS >= E: {errs} of bar 1e-10; two engines {np.abs(outs[0] - outs[1]).max():.3e} of bar 1e-12")
    assert max(errs) <= 1e-10 and np.abs(outs[0] - outs[1]).max() <= 1e-12
    few = edges[:8]
    eng = _engine(n, D, few, k=8, S=4)
    try:
        eng.set_positions(pos)
        with pytest.raises(RuntimeError):
            eng.step(np.arange(4, dtype=np.int32))
    finally:
        eng.close()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 300001])
def test_float32_accessors_of_a_float64_handle(count):
    """gh_set_positions / gh_get_positions on a float64 handle convert on the device (gh_f64_set_positions_f32,
    gh_f64_get_positions_f32): floats widen exactly, doubles round to nearest as astype(float32) does."""
    from graphem_rapids_amd._native import ptr
    n, D = (count, 1) if count % 3 else (count // 3, 3)
    edges = np.array([[0, n - 1]], dtype=np.int32)
    rng = np.random.default_rng(count)
    eng = _engine(n, D, edges)
    try:
        f = (rng.standard_normal((n, D)) * 10.0 ** rng.integers(-20, 20, (n, D))).astype(np.float32)
        eng._chk(eng.lib.gh_set_positions(eng.handle, ptr(f)))
        assert np.array_equal(eng.get_positions(), f.astype(np.float64))
        d = rng.standard_normal((n, D)) * 10.0 ** rng.integers(-30, 30, (n, D))
        d.flat[0] = 1.0 + 2.0 ** -24                    # a tie of the rounding: to even
        eng.set_positions(d)
        got = np.full((n, D), np.nan, dtype=np.float32)
        eng._chk(eng.lib.gh_get_positions(eng.handle, ptr(got)))
        assert np.array_equal(got, d.astype(np.float32))
    finally:
        eng.close()


@pytest.mark.slow
def test_one_step_at_one_million_vertices():
    """1 M vertices, 4 M edges, D = 3, k = 10, S = 64: filtered search with the matrix-pipe pre-filter, spring4<3>, mid4<3>
    and update loops of several trips in one step.  The engine's rows against the brute force, then the step on those
    rows against the reference."""
    import graphem_rapids_amd as gra
    n, D, k, S = 1000000, 3, 10, 64
    edges = np.ascontiguousarray(gra.random_regular_edges(n, 8, seed=2), dtype=np.int32)
    E = len(edges)
    rng = np.random.default_rng(11)
    pos = rng.standard_normal((n, D))
    sampled = rng.permutation(E)[:S].astype(np.int32)
    mid = np.asarray(reference.midpoints(pos, edges), dtype=np.float64)
    assert reference.knn_gap(mid, sampled, k) >= 1e-9
    rows = reference.knn_rows(mid, sampled, k)
    eng = _engine(n, D, edges, k=k, S=S)
    try:
        eng.set_positions(pos)
        knn = eng.knn_midpoints(sampled)
        eng.step(sampled)
        out = eng.get_positions()
    finally:
        eng.close()
    assert np.array_equal(knn, rows)
    err = _abs(out, reference.step(pos, edges, sampled, rows, *PRM))
    print(f"\none step at n={n}: {err:.3e} of bar 1e-10")
    assert err <= 1e-10
