"""Anchors tests/f32_reference.py -- what tests/test_hip_f32_phases.py compares the float32 engine's intersection and update
phases with -- without a GPU: the restated update against the float32 golden fixtures, the C oracle and a model of the
kernels' one-pass double statistics; the unrolled intersection sum against the oracle and the extended-precision reference;
and every condition the GPU tests put on their inputs, computed from the oracle and the restatement alone."""
import numpy as np
import pytest

import f32_reference as ref
import f64_reference
import oracle
from conftest import GOLDEN_CASES, load_golden

L_MIN, K_ATTR, K_INTER = ref.PRM


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_update_reproduces_the_golden_fixtures_and_the_oracle(case):
    """pos_next_t of every captured step, and oracle.integrate_normalise on the same forces, within the existing 2e-6."""
    g = load_golden(case)
    worst = 0.0
    for t in g["steps"]:
        pos, Fs, Fi = g[f"pos_{t}"], g[f"F_spring_{t}"], g[f"F_inter_{t}"]
        assert pos.dtype == np.float32
        out, bar = ref.update(pos, Fs, Fi)
        assert out.dtype == np.float32 and bar.shape == out.shape and (bar > 0).all()
        worst = max(worst, float(np.abs(out - g[f"pos_next_{t}"]).max()),
                    float(np.abs(out - oracle.integrate_normalise(pos, Fs, Fi)).max()))
    print(f"\n{case}: restated update vs fixtures and oracle: {worst:.3e} of 2e-6")
    assert worst <= 2e-6


def test_bar_is_a_few_float32_ulps_on_a_plain_cloud():
    """On a standard Gaussian cloud the bar is a handful of ulps of the result: between 1 and 6 ulp(max(|out|, 1))."""
    pos = ref.start_state("gauss", 20001, 3, 1)
    Fs, Fi = ref.injected_forces(pos, 2)
    out, bar = ref.update(pos, Fs, Fi)
    unit = ref.ulp32(np.maximum(np.abs(out), 1.0))
    assert (bar >= ref.ulp32(out)).all() and (bar <= 6 * unit).all()


@pytest.mark.parametrize("n,D,start", [c for c in ref.UPDATE_CASES if c[0] <= 20001]
                         + [pytest.param(*c, marks=pytest.mark.slow) for c in ref.UPDATE_CASES if c[0] > 20001])
def test_update_agrees_with_the_one_pass_double_model(n, D, start):
    """The starts of the GPU update tests: a numpy model of the kernels' statistics (float64 sums of x and x^2, one pass)
    lies within the bar of the restatement, and a constant column comes out as exact zeros."""
    pos = ref.start_state(start, n, D, 100 * D + len(start))
    Fs, Fi = ref.injected_forces(pos, n + D)
    assert (Fi.any(axis=1).sum() == max(1, n // 20))
    out, bar = ref.update(pos, Fs, Fi)
    model = ref.one_pass_model(ref.integrate(pos, Fs, Fi))
    frac = ref.fraction(model, out, bar)
    print(f"\nupdate n={n} D={D} {start}: one-pass model at {frac:.3f} of the bar")
    assert np.isfinite(out).all() and frac <= 1.0
    if start == "constant":
        assert not out[:, D - 1].any() and not model[:, D - 1].any()
    if n >= 257 and start == "gauss":
        o64 = out.astype(np.float64)
        assert np.abs(o64.mean(axis=0)).max() <= 1e-4 and np.abs(o64.std(axis=0, ddof=1) - 1.0).max() <= 1e-4


def test_update_stats_from_moves_when_the_statistics_lose_the_intersection_forces():
    pos = ref.start_state("gauss", 20001, 3, 5)
    Fs, Fi = ref.injected_forces(pos, 6)
    out, bar = ref.update(pos, Fs, Fi)
    same, _ = ref.update_stats_from(pos, Fs, Fi, Fi)
    assert np.array_equal(same, out)
    lost, _ = ref.update_stats_from(pos, Fs, Fi, np.zeros_like(Fi))
    assert ref.fraction(lost, out, bar) > 10.0


@pytest.mark.parametrize("D", ref.PLANTED_DIMS)
def test_intersection_sum_on_the_planted_pairs(D):
    """The unrolled sum agrees with the oracle within the existing rtol 1e-6 and with the extended-precision reference on
    the same float32 positions within 1e-6 relative; the conditions of the GPU test hold: counts equal PLANTED_COUNTS,
    touching, collinear, shared-vertex and i > j pairs are present, the hub receives at least 200 terms."""
    pos, edges, sampled, knn, hub = ref.planted(D)
    exact, sum_abs, touched = ref.intersection_sum(pos, edges, sampled, knn, K_INTER)
    assert exact.shape == pos.shape and exact.dtype == ref.LD
    if D == 1:
        assert not exact.any() and not touched.any()
        return
    counts = ref.classify_planted(pos, edges, sampled, knn, hub)
    assert counts == ref.PLANTED_COUNTS
    assert min(counts["touching"], counts["collinear"], counts["shared"], counts["i_gt_j"]) >= 1 and counts["hub"] >= 200
    ends, terms, i, j = ref.unrolled_terms(pos, edges, sampled, knn, K_INTER)
    assert len(i) == counts["listed"] - counts["i_gt_j"] - counts["shared"] == 946
    crossing = terms.reshape(len(ends), -1).any(axis=1)
    assert crossing.sum() == ref.crossing_count(pos, edges, sampled, knn) == counts["crossing"] == 886
    assert ((ends[crossing] == hub).any(axis=1)).sum() == counts["hub"]
    orc = oracle.intersection_forces(pos, edges, sampled, knn, K_INTER)
    assert np.array_equal(orc.any(axis=1), touched)
    scale = max(1.0, float(np.abs(orc).max()))
    e64 = exact.astype(np.float64)
    np.testing.assert_allclose(orc, e64, rtol=1e-6, atol=1e-6 * scale)
    f64 = f64_reference.intersection_forces(pos, edges, sampled, knn, K_INTER)
    rel = float(np.abs(f64 - exact).max()) / scale
    bar = ref.intersection_bar(exact, sum_abs)
    print(f"\nplanted D={D}: oracle at {ref.fraction(orc, e64, bar):.1f} bars of the exact sum (its own float32 summation), "
          f"long-double reference {rel:.2e} relative")
    assert rel <= 1e-6 and (bar > 0)[touched].all()


def test_unrolled_terms_are_what_the_oracle_adds_up():
    """A vertex that one pair touches holds that pair's term in the oracle's own output, bit for bit."""
    n, D, edges, pos, k, S, samples, kw, rows = ref.step_case("per_query")
    knn = rows(pos, edges, samples[0], k)
    ends, terms, _, _ = ref.unrolled_terms(pos, edges, samples[0], knn)
    crossing = terms.reshape(len(ends), -1).any(axis=1)
    hits = np.bincount(ends[crossing].reshape(-1), minlength=n)
    orc = oracle.intersection_forces(pos, edges, samples[0], knn, K_INTER)
    once = 0
    for p in np.flatnonzero(crossing):
        for r in range(4):
            if hits[ends[p, r]] == 1:
                assert np.array_equal(orc[ends[p, r]], terms[p, r])
                once += 1
    assert once >= 100


@pytest.mark.parametrize("name", list(ref.NOSAMPLE_CASES))
def test_graphs_of_the_update_inside_a_step(name):
    """The graphs have what their names say: row strides 4, 8, 16 and 20; more than 256 workgroups of 256 rows for "many*"
    (stats_reduce_kernel's second trip); hubs of 5000 edges or more.  (Without sampling no graph takes the fused route.)"""
    n, edges = ref.nosample_graph(name)
    D = ref.NOSAMPLE_CASES[name][1]
    assert edges.max() < n and (n > 256 * 256) == name.startswith("many")
    assert ref.row_stride(D) == {"many4": 4, "many8": 8, "many16": 16}.get(name, ref.row_stride(D))
    assert ref.row_stride(D) == {"unfused4": 4, "unfused8": 8, "unfused16": 16, "general": 20}.get(name, ref.row_stride(D))
    if name in ("hubs", "ladder"):
        assert np.bincount(edges.ravel()).max() >= 5000
    pos = ref.start_state("constant", n, D, 1)
    assert not oracle.spring_forces(pos, edges, L_MIN, K_ATTR)[:, D - 1].any()     # no spring force along a constant column


@pytest.mark.parametrize("name", list(ref.STEP_CASES))
def test_whole_step_inputs_meet_their_conditions(name):
    """Both steps of every whole-step case of the GPU file (the second from the restatement's own first output): at least
    200 crossing pairs, at least 5 % of the vertices touched, and statistics that lost the intersection forces lie more than
    ten bars away; the oracle's own sum lies within the existing rtol 1e-6 of the exact one."""
    n, D, edges, pos, k, S, samples, kw, rows = ref.step_case(name)
    assert not np.array_equal(samples[0], samples[1])
    for t in range(2):
        Fs = oracle.spring_forces(pos, edges, L_MIN, K_ATTR)
        knn = rows(pos, edges, samples[t], k)
        cond, (Fi, out, bar) = ref.step_conditions(pos, edges, samples[t], knn, Fs)
        print(f"\n{name} step {t}: crossing {cond[0]}, touched {cond[1]:.3f}, lost statistics at {cond[2]:.3g} bars")
        ref.assert_step_conditions(cond, (name, t))
        orc = oracle.intersection_forces(pos, edges, samples[t], knn, K_INTER)
        np.testing.assert_allclose(orc, Fi, rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(orc).max())))
        pos = out
    for other in ref.PARTITION_CASES:
        assert other in ref.STEP_CASES
