"""The float32 engine's intersection and update phases against tests/f32_reference.py -- given float32 inputs both have an
essentially exact answer (anchored without a GPU by tests/test_f32_reference_cpu.py) -- at the shapes and routes the kernels
branch on.  Which kernel or call site each test names:

  intersect_kernel<2..16> (gh_intersect_pair_t), <0> at D = 17, 20, 40      test_intersection_forces_on_planted_pairs
  (gh_intersect_pair, scratch), D = 1; inter_to_dense, inter_cleanup        (each case called twice: the second rests on the clean-up)
  integrate_given_kernel + column_stats_kernel + normalise_kernel<4,8,16,0> test_integrate_normalise_alone
  grid below / at the 2048-workgroup cap, n = 2, 3, n % 256 != 0
  integrate_kernel<4>, <8>, <16> + stats_reduce_kernel (one trip)           test_update_inside_a_step[unfused4 / 8 / 16]
  the same with 274 workgroups (stats_reduce_kernel's second trip)          test_update_inside_a_step[many4 / 8 / 16]
  integrate_generic_kernel + column_stats_kernel, normalise_kernel<0>       test_update_inside_a_step[general]
  long-row spring kernels feeding the update; pad columns of the rows       test_update_inside_a_step[hubs, ladder]; every case
  (a step with sample_size = 0 never runs the fused kernel, whatever the number of edges: stats_fix_kernel is below)
  knn_block_select_kernel -> gh_intersect_query_wide<5, 8>                  test_whole_step[per_query]
  knn_block_select_kernel -> gh_intersect_pair (D > 16, scratch)            test_whole_step[per_query_general]
  knn_select_kernel -> gh_intersect_query_wide<3, 4>, unfused scan          test_whole_step[scan4_unfused]
  knn_select_kernel -> gh_intersect_query_wide<8, 8>, <16, 16>;             test_whole_step[wide8, wide16]
  stats_fix_kernel<8>, <16> with skip_reduce = 1
  knn_block_select_sort_kernel (K > 128) selects, intersect_kernel<3>       test_whole_step[sort]
  runs the pairs in a launch of its own
  fused spring+scan, select launch reduces: stats_fix_kernel<4>,            test_whole_step[fused]
  skip_reduce = 1
  knn_select_wave_kernel (S >= 2048) -> gh_intersect_query_wide, per-query  test_whole_step[wave, wave8, wave16]
  touched runs; stats_fix_kernel<4>, <8>, <16> with skip_reduce = 0
  knn_select_cdist_kernel (knn_distance="cdist")                            test_whole_step[cdist]
  grid search (exists for D <= 3 only) / exact inverted file at D = 3, 6    test_whole_step[grid3, ivf3, ivf6]
  -> knn_select_kernel
  knn_merge_kernel -> gh_intersect_query_wide with own_lo / own_hi;         test_partitioned_finishes[fused-*, wide8-*]
  gh_norm_src: form C (own, packed and not), form B (gathered), form D (overlap)
  knn_merge_kernel -> gh_intersect_pair_t<3, 4> (k >= 128: its only         test_partitioned_finishes[sort-2-*]
  reachable use inside intersect_query), own_lo / own_hi
  (gh_intersect_pair_any has no caller.)

Bars: f32_reference.update's per-element bar and f32_reference.intersection_bar (derived in that module, not measured).
Every test prints its worst error as a fraction of its bar.  Needs a real MI355X."""
import numpy as np
import pytest

import f32_reference as ref
import oracle

pytestmark = pytest.mark.gpu

L_MIN, K_ATTR, K_INTER = ref.PRM


def _engine(n, D, edges, k=10, S=0, **kw):
    from graphem_rapids_amd import _native
    return _native.Engine(n, D, edges, *ref.PRM, k, S, **kw)


def _device_rows(eng):
    """The engine's position rows as stored: (n, row stride), vertex order as given (reorder off or identity)."""
    import torch
    from graphem_rapids_amd.embedder_hip import device_view
    dev = torch.device("cuda", 0)
    eng.sync()
    v = device_view(eng.positions_device_ptr(), (eng.positions_rows_allocated(), eng.ld), torch.float32, dev, eng)
    return v[: eng.n].cpu().numpy()


def _check_intersection(F, exact, sum_abs, touched, what):
    bar = ref.intersection_bar(exact, sum_abs)
    frac = ref.fraction(F, exact.astype(np.float64), bar)
    print(f"\n{what}: intersection forces at {frac:.3f} of the bar (max|F| {float(np.abs(exact).max()):.3g})")
    assert F.dtype == np.float32 and frac <= 1.0, (what, frac)
    assert np.array_equal(F.any(axis=1), touched), what
    return frac


# ---- a. per-phase intersection forces on the planted pairs ------------------------------------------------------------

@pytest.mark.parametrize("D", ref.PLANTED_DIMS)
def test_intersection_forces_on_planted_pairs(D):
    """One case per instantiation of intersect_kernel (D = 2..16), the scratch form (17, 20, 40) and D = 1 (zeros), on
    f64_reference.planted_intersections in float32: 886 listed crossings, 912 pairs with i > j, 30 touching, 30 collinear
    and 30 sharing a vertex -- none of which may push -- and a hub 256 terms add to.  Twice in a row: the second call
    starts from what inter_cleanup left."""
    pos, edges, sampled, knn, hub = ref.planted(D)
    exact, sum_abs, touched = ref.intersection_sum(pos, edges, sampled, knn, K_INTER)
    if D >= 2:       # the conditions on the input, on the reference alone
        counts = ref.classify_planted(pos, edges, sampled, knn, hub)
        assert counts == ref.PLANTED_COUNTS and counts["hub"] >= 200
        assert min(counts["touching"], counts["collinear"], counts["shared"], counts["i_gt_j"]) >= 1
        assert ref.crossing_count(pos, edges, sampled, knn) == counts["crossing"]
        ends, terms, _, _ = ref.unrolled_terms(pos, edges, sampled, knn, K_INTER)
        assert (terms.reshape(len(ends), -1).any(axis=1) & (ends == hub).any(axis=1)).sum() >= 200
    else:
        assert not exact.any()
    eng = _engine(len(pos), D, edges, k=ref.PLANTED_K, S=len(sampled))
    try:
        eng.set_positions(pos)
        F = eng.intersection_forces(sampled, knn)
        again = eng.intersection_forces(sampled, knn)
    finally:
        eng.close()
    _check_intersection(F, exact, sum_abs, touched, f"planted D={D}")
    _check_intersection(again, exact, sum_abs, touched, f"planted D={D}, second call")
    assert np.array_equal(F, again)
    if D == 1:
        assert not F.any()
        return
    hub_bar = ref.intersection_bar(exact[hub], sum_abs[hub])
    hub_frac = ref.fraction(F[hub], exact[hub].astype(np.float64), hub_bar)
    print(f"planted D={D}: hub row at {hub_frac:.3f} of the bar (|F| {float(np.abs(exact[hub]).max()):.3g})")
    assert F[hub].any() and hub_frac <= 1.0


# ---- b. integrate_normalise alone -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,D,start", [c if c[0] < 500000 else pytest.param(*c, marks=pytest.mark.slow) for c in ref.UPDATE_CASES])
def test_integrate_normalise_alone(n, D, start):
    """gh_integrate_normalise (integrate_given_kernel + column_stats_kernel + normalise_kernel) with injected forces: row
    strides 4, 8, 16 and the general one, n LD on both sides of 8 388 608 (the 2048-workgroup cap of the normalise grid),
    n = 2 and 3, n not a multiple of 256 (column_stats_kernel's stride), every start of f32_reference.STARTS.  Fi is zero
    except on 5 % of the rows.  A constant column comes out as exact zeros; the call restores the positions it normalised
    over (so the pad columns normalise_kernel writes are not visible here: test_update_inside_a_step reads them)."""
    pos = ref.start_state(start, n, D, 100 * D + len(start))
    Fs, Fi = ref.injected_forces(pos, n + D)
    out, bar = ref.update(pos, Fs, Fi)
    edges = np.stack([np.arange(min(n, 65) - 1), np.arange(1, min(n, 65))], axis=1).astype(np.int32)
    eng = _engine(n, D, edges)
    try:
        assert eng.ld == ref.row_stride(D)
        eng.set_positions(pos)
        got = eng.integrate_normalise(Fs, Fi)
        after = eng.get_positions()
    finally:
        eng.close()
    frac = ref.fraction(got, out, bar)
    print(f"\nintegrate_normalise n={n} D={D} {start}: {frac:.3f} of the bar")
    assert got.dtype == np.float32 and np.isfinite(got).all() and frac <= 1.0
    assert np.array_equal(after, pos)
    if start == "constant":
        assert not got[:, D - 1].any()


# ---- c. the update inside step(), sample_size = 0 -------------------------------------------------------------------

@pytest.mark.parametrize("start", ref.STARTS)
@pytest.mark.parametrize("name", list(ref.NOSAMPLE_CASES))
def test_update_inside_a_step(name, start):
    """Three steps without an intersection phase on the routes gh_launch_integrate has for such a step (the table at the
    top; the fused route is not among them).  Fs is oracle.spring_forces, which the engine's must equal bit for bit; every step is compared with the
    restatement started from the engine's own previous output.  Pad columns of the stored rows stay exact zeros."""
    n, edges = ref.nosample_graph(name)
    D = ref.NOSAMPLE_CASES[name][1]
    pos = ref.start_state(start, n, D, 7 * D + len(start))
    eng = _engine(n, D, edges, k=10, S=0, reorder="off")
    worst = 0.0
    try:
        eng.set_positions(pos)
        for t in range(3):
            Fs = oracle.spring_forces(pos, edges, L_MIN, K_ATTR)
            assert np.array_equal(eng.spring_forces(), Fs), (name, start, t)
            out, bar = ref.update(pos, Fs, np.zeros_like(Fs))
            eng.step()
            got = eng.get_positions()
            frac = ref.fraction(got, out, bar)
            worst = max(worst, frac)
            assert np.isfinite(got).all() and frac <= 1.0, (name, start, t, frac)
            if start == "constant":
                assert not got[:, D - 1].any()
            pos = got
        rows = _device_rows(eng)
    finally:
        eng.close()
    print(f"\nupdate inside a step {name} D={D} {start}: {worst:.3f} of the bar over three steps")
    assert np.array_equal(rows[:, :D], pos) and not rows[:, D:].any()


# ---- d. a whole step with the intersection phase ----------------------------------------------------------------------

def _step_reference(pos, edges, sampled, knn, what):
    """Conditions on the input and (Fs, exact, sum_abs, touched, out, bar) of one whole step."""
    Fs = oracle.spring_forces(pos, edges, L_MIN, K_ATTR)
    cond, (Fi, out, bar) = ref.step_conditions(pos, edges, sampled, knn, Fs)
    print(f"\n{what}: crossing {cond[0]}, touched {cond[1]:.3f}, lost statistics at {cond[2]:.3g} bars")
    ref.assert_step_conditions(cond, what)
    exact, sum_abs, touched = ref.intersection_sum(pos, edges, sampled, knn, K_INTER)
    return Fs, exact, sum_abs, touched, out, bar


@pytest.mark.parametrize("name", list(ref.STEP_CASES))
def test_whole_step(name):
    """Two steps with different samples; the second runs from the first's output and is what catches an accumulator or flag
    that was not cleared.  Per step: the engine's neighbour rows equal the oracle's; the per-phase intersection forces lie
    within their bar; step(sampled) equals update(pos, Fs, Fi) within its bar, Fi being what the per-phase call returned.
    (The conditions on the input are computed with the exact sum rounded to float32 in its place.)"""
    n, D, edges, pos, k, S, samples, kw, rows_of = ref.step_case(name)
    eng = _engine(n, D, edges, k=k, S=S, **kw)
    worst = [0.0, 0.0]
    try:
        eng.set_positions(pos)
        for t in range(2):
            what = f"whole step {name} D={D} step {t}"
            knn = rows_of(pos, edges, samples[t], k)
            assert np.array_equal(eng.knn_midpoints(samples[t]), knn), what
            Fs, exact, sum_abs, touched, out, bar = _step_reference(pos, edges, samples[t], knn, what)
            assert np.array_equal(eng.spring_forces(), Fs), what
            Fi = eng.intersection_forces(samples[t], knn)
            worst[0] = max(worst[0], _check_intersection(Fi, exact, sum_abs, touched, what))
            out, bar = ref.update(pos, Fs, Fi)
            eng.step(samples[t])
            got = eng.get_positions()
            frac = ref.fraction(got, out, bar)
            worst[1] = max(worst[1], frac)
            print(f"{what}: positions at {frac:.3f} of the bar")
            assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
            pos = got
    finally:
        eng.close()
    print(f"whole step {name}: intersection {worst[0]:.3f}, positions {worst[1]:.3f} of their bars")


# ---- e. the partitioned finishes on one GPU ---------------------------------------------------------------------------

def _partitioned_steps(finish, world, n, D, edges, pos, k, S, samples, packed=None):
    """The in-process harness of test_hip_parity.test_random_partitioned_configurations: `world` engines on one GPU, the
    collectives emulated with device copies.  Yields every rank's positions after each step."""
    import torch
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import HipShardEngine, partition_rows, step_in_process
    shards = []
    for r in range(world):
        chunk, lo, hi = partition_rows(n, world, r)
        sh = HipShardEngine(n, D, edges, *ref.PRM, k, S, 7, (lo, hi, 0, 0, _native.EDGES_HASHED), 0)
        if finish == "own":
            sh.rank_layout(world, r, chunk, packed=packed)
        elif finish == "overlap":
            sh.overlap_layout(world, r, chunk)
        else:
            sh.gather_layout(world, r, chunk)
        sh.set_positions(pos)
        shards.append(sh)
    try:
        for sampled in samples:
            order = []
            step_in_process(shards, finish, sampled, after={x: (lambda x=x: order.append(x)) for x in ("rows", "keys")})
            assert order == (["rows", "keys"] if finish == "overlap" else ["keys"])   # form D: every rank's rows went early
            if finish == "own":
                assert (shards[0].packed_blocks is not None) == bool(packed and D < shards[0].ld)
            torch.cuda.synchronize()
            yield [sh.get_positions() for sh in shards]
    finally:
        for sh in shards:
            sh.eng.close()


@pytest.mark.parametrize("finish", ["own", "own_packed", "gathered", "overlap"])
@pytest.mark.parametrize("name,world", [(c, w) for c, ws in ref.PARTITION_CASES.items() for w in ws])
def test_partitioned_finishes(name, world, finish):
    """Forms C (own rows, with and without the unpadded block exchange), B (gathered) and D (overlap: patch lists, rows of D
    floats) on 2, 3 and 5 row partitions, from a whole-step state at D = 3 and one at D = 8, two steps.  Every rank's output
    lies within the bar of update(...) started from the ranks' own previous output (Fi: the exact sum rounded to float32 -- a
    partitioned engine has no per-phase call), and the ranks agree bit for bit: that gh_norm_src walks blocks, row strides and
    every rank's statistics block.  The k = 130 state on two ranks runs its pairs through gh_intersect_pair_t in the merge
    kernel, the one place that reaches it."""
    n, D, edges, pos, k, S, samples, kw, rows_of = ref.step_case(name)
    packed = finish == "own_packed"
    steps = _partitioned_steps("own" if packed else finish, world, n, D, edges, pos, k, S, samples,
                               packed=(packed if finish.startswith("own") else None))
    worst = 0.0
    for t, outs in enumerate(steps):
        what = f"partitioned {finish} world={world} {name} D={D} step {t}"
        knn = rows_of(pos, edges, samples[t], k)
        Fs, exact, sum_abs, touched, out, bar = _step_reference(pos, edges, samples[t], knn, what)
        for r, got in enumerate(outs):
            frac = ref.fraction(got, out, bar)
            worst = max(worst, frac)
            assert np.isfinite(got).all() and frac <= 1.0, (what, r, frac)
            assert np.array_equal(got, outs[0]), (what, r)
        pos = outs[0]
    print(f"partitioned {finish} world={world} {name}: {worst:.3f} of the bar")
