"""Rank correlation without a GPU (csrc/correlation.hip host path, graphem-rapids_amd/visualization.py): the library's
host path against the restatement of the header's rules (tests/correlation_reference.py) bit for bit, against the
reference's own procedure (scipy.stats.spearmanr on the materialised resample, pandas' Spearman matrix), the p-value,
the four report functions, the errors, and benchmark_correlations' new keywords.

Tolerance against scipy: 8 * n * 2**-53.  Our rho is a few roundings away from the exact quotient of integers; scipy
forms the same quotient as a normalised dot product of n floating-point terms, whose summation error is bounded by a
small multiple of n * 2**-53.  The difference is therefore scipy's own error.
"""
import math
import os
import warnings

import numpy as np
import pytest
from scipy import special, stats

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
import correlation_reference as ref

CORR_SYMBOLS = ["gh_corr_create", "gh_corr_destroy", "gh_corr_last_error", "gh_corr_set_memory_budget", "gh_corr_rho",
                "gh_corr_matrix", "gh_corr_bootstrap"]
GRID_N = [2, 3, 50, 500, 5000]
GRID_REPS = 32
GRID_SEED = 11
KINDS = ["continuous", "rounded", "degrees", "two_valued", "constant", "signed_zeros", "monotone", "anti_monotone", "noisy"]
# every kind occurs; (continuous, monotone) and (continuous, anti_monotone) are the perfectly monotone pairs
GRID_PAIRS = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (1, 2), (2, 3), (5, 8), (8, 1), (3, 3), (4, 2)]


def grid_columns(n):
    """(len(KINDS), n) float64: the column kinds of the check grid."""
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal(n)
    noisy = x + rng.standard_normal(n)
    zeros = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    zeros[rng.random(n) < 0.3] = 1.5
    zeros[rng.random(n) < 0.2] = -2.0
    zeros[0], zeros[-1] = -0.0, 0.0
    cols = {
        "continuous": x,
        "rounded": np.round(noisy, 1),
        "degrees": np.floor(np.exp(rng.standard_normal(n)) * 3 + 1),
        "two_valued": (rng.random(n) < 0.3).astype(np.float64),
        "constant": np.full(n, 4.25),
        "signed_zeros": zeros,
        "monotone": np.exp(x) * 3 - 1,
        "anti_monotone": -x ** 3,
        "noisy": noisy,
    }
    return np.stack([cols[k] for k in KINDS])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def close_or_both_nan(ours, theirs, tol):
    ours, theirs = np.asarray(ours, dtype=np.float64), np.asarray(theirs, dtype=np.float64)
    nan = np.isnan(theirs)
    return np.array_equal(np.isnan(ours), nan) and bool(np.all(np.abs(ours[~nan] - theirs[~nan]) <= tol))


def scipy_rho(x, y):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return stats.spearmanr(x, y)[0]


def check_against_restatement(device_id, n):
    """Triples and rho of the library (host path or device) == the restatement, plain and for every replicate."""
    cols = grid_columns(n)
    corr = _native.Correlation(cols, device_id)
    matrix, sums = corr.matrix(sums=True)
    rep, rep_sums = corr.bootstrap(GRID_PAIRS, GRID_REPS, GRID_SEED, sums=True)
    corr.close()
    m = len(KINDS)
    every = [(x, y) for x in range(m) for y in range(m)]
    want = ref.triples(cols, every, np.ones(n, dtype=np.int64))
    for (x, y), t in zip(every, want):
        assert tuple(int(v) for v in sums[x, y]) == t, (n, KINDS[x], KINDS[y])
        want_rho = (math.nan if t[1] == 0 else 1.0) if x == y else ref.rho_of(*t)
        assert same_bits(matrix[x, y], want_rho), (n, KINDS[x], KINDS[y])
    for b in range(GRID_REPS):
        want = ref.triples(cols, GRID_PAIRS, ref.multiplicities(n, b, GRID_SEED))
        for p, t in enumerate(want):
            assert tuple(int(v) for v in rep_sums[p, b]) == t, (n, GRID_PAIRS[p], b)
            assert same_bits(rep[p, b], ref.rho_of(*t)), (n, GRID_PAIRS[p], b)


def test_symbols_declared_and_bound():
    lib = _native.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "graphem_hip.h")).read()
    for name in CORR_SYMBOLS:
        assert name + "(" in header, name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name


def test_exports():
    for name in ["spearman_matrix", "bootstrap_spearman", "report_corr", "report_full_correlation_matrix",
                 "plot_radial_vs_centrality", "display_benchmark_results"]:
        assert name in gr.__all__ and callable(getattr(gr, name)), name


@pytest.mark.parametrize("n", GRID_N)
def test_host_path_equals_restatement(n):
    check_against_restatement(-1, n)


def test_resample_is_a_resample():
    for n in (2, 3, 50, 5000):
        c = ref.multiplicities(n, 3, 9)
        assert c.sum() == n and c.min() >= 0


@pytest.mark.parametrize("n", GRID_N)
def test_host_path_against_scipy_on_materialised_resamples(n):
    cols = grid_columns(n)
    tol = 8 * n * 2.0 ** -53
    pairs = [(0, j) for j in range(1, len(KINDS))] + [(1, 2), (5, 8)]
    corr = _native.Correlation(cols, -1)
    matrix = corr.matrix()
    rep = corr.bootstrap(pairs, GRID_REPS, GRID_SEED)
    corr.close()
    for p, (x, y) in enumerate(pairs):
        assert close_or_both_nan(matrix[x, y], scipy_rho(cols[x], cols[y]), tol), (n, KINDS[x], KINDS[y])
        for b in range(GRID_REPS):
            idx = ref.resample_indices(n, b, GRID_SEED)
            assert close_or_both_nan(rep[p, b], scipy_rho(cols[x][idx], cols[y][idx]), tol), (n, KINDS[x], KINDS[y], b)


@pytest.mark.parametrize("n", GRID_N)
def test_matrix_against_pandas(n):
    import pandas as pd
    cols = grid_columns(n)
    ours = gr.spearman_matrix(cols, device_id=-1)
    theirs = pd.DataFrame(cols.T).corr(method="spearman").to_numpy()
    assert ours.shape == (len(KINDS), len(KINDS)) and np.array_equal(np.isnan(ours), np.isnan(ours.T))
    assert close_or_both_nan(ours, theirs, 8 * n * 2.0 ** -53)
    const = KINDS.index("constant")
    assert np.isnan(ours[const]).all() and np.isnan(ours[:, const]).all()
    for k in range(len(KINDS)):          # at n = 2 or 3 a column of few values can come out constant too
        assert np.isnan(ours[k, k]) if np.all(cols[k] == cols[k][0]) else ours[k, k] == 1.0, KINDS[k]
    assert ours[0, KINDS.index("monotone")] == 1.0 and ours[0, KINDS.index("anti_monotone")] == -1.0


def scipy_formula_p(rho, n):
    dof = n - 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = rho * np.sqrt((dof / ((rho + 1.0) * (1.0 - rho))).clip(0))
    return 2 * special.stdtr(dof, -np.abs(t))


@pytest.mark.parametrize("n", [50, 500, 5000])
def test_p_value(n):
    cols = grid_columns(n)
    compared = 0
    for j in range(1, len(KINDS)):
        rho, p, _, _, _ = gr.bootstrap_spearman(cols[0], [cols[j]], reps=2, seed=0, device_id=-1)
        assert same_bits(p[0], scipy_formula_p(rho[0], n)), KINDS[j]
        if not math.isnan(rho[0]) and abs(rho[0]) < 0.99:
            theirs = stats.spearmanr(cols[0], cols[j]).pvalue
            assert abs(p[0] - theirs) <= 1e-6 * abs(theirs), (KINDS[j], p[0], theirs)
            compared += 1
    assert compared >= 5


def test_report_corr(capsys):
    cols = grid_columns(500)
    x, y = cols[0], cols[KINDS.index("rounded")]
    rho, p = gr.report_corr("Degree", x, y, reps=200, seed=5)
    line = capsys.readouterr().out
    r, pp, lo, hi, rep = gr.bootstrap_spearman(x, [y], reps=200, seed=5)
    assert (rho, p) == (r[0], pp[0]) and isinstance(rho, float) and isinstance(p, float)
    assert abs(rho - stats.spearmanr(x, y)[0]) <= 8 * 500 * 2.0 ** -53
    assert rep.shape == (1, 200)
    assert lo[0] == np.percentile(rep[0], 2.5) and hi[0] == np.percentile(rep[0], 97.5)
    assert line == f"{'Degree':15s}: rho = {rho:.3f} (95% CI: [{lo[0]:.3f}, {hi[0]:.3f}]), p = {p:.6f}\n"
    gr.report_corr("Degree", x, y, reps=200, seed=5)
    assert capsys.readouterr().out == line
    other = gr.bootstrap_spearman(x, [y], reps=200, seed=6)[4]
    assert not np.array_equal(other, rep)
    assert np.array_equal(gr.bootstrap_spearman(x, [y], reps=200, seed=5)[4], rep)
    lo10, hi10 = gr.bootstrap_spearman(x, [y], reps=200, seed=5, alpha=0.1)[2:4]
    assert lo10[0] == np.percentile(rep[0], 10) and hi10[0] == np.percentile(rep[0], 90)


def test_bootstrap_does_not_touch_numpy_global_state():
    cols = grid_columns(50)
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    gr.bootstrap_spearman(cols[0], [cols[1]], reps=8)
    assert np.array_equal(np.random.get_state()[1], before)


def test_report_full_correlation_matrix(capsys):
    import pandas as pd
    cols = grid_columns(500)
    seven = [cols[KINDS.index(k)] for k in ["continuous", "degrees", "signed_zeros", "noisy", "monotone", "rounded", "two_valued"]]
    frame = gr.report_full_correlation_matrix(*seven, reps=100, seed=2)
    out = capsys.readouterr().out.splitlines()
    labels = ["Radius", "Degree", "Betweenness", "Eigenvector", "PageRank", "Closeness", "Node Load"]
    assert isinstance(frame, pd.DataFrame) and frame.shape == (7, 7)
    assert list(frame.index) == labels and list(frame.columns) == labels
    values = frame.to_numpy()
    assert np.array_equal(values, values.T) and np.all(np.diag(values) == 1.0)
    theirs = pd.DataFrame(dict(zip(labels, seven))).corr(method="spearman").to_numpy()
    assert np.abs(values - theirs).max() <= 8 * 500 * 2.0 ** -53
    assert out[0] == "Correlations with radial distance:" and len(out) == 7
    rho, p, lo, hi, _ = gr.bootstrap_spearman(seven[0], seven[1:], reps=100, seed=2)
    for j, name in enumerate(labels[1:]):
        assert out[1 + j] == f"{name:15s}: rho = {rho[j]:.3f} (95% CI: [{lo[j]:.3f}, {hi[j]:.3f}]), p = {p[j]:.6f}"


def test_display_benchmark_results():
    rows = [{"time": 1.0, "extra": 3, "n": 10, "graph_type": "ba", "influence": 4.0, "seed_method": "graphem", "m": 20},
            {"time": 2.0, "extra": 4, "n": 11, "graph_type": "ws", "influence": 5.0, "seed_method": "greedy", "m": 22}]
    frame = gr.display_benchmark_results(rows)
    assert list(frame.columns) == ["graph_type", "n", "m", "seed_method", "influence", "time"]
    assert list(frame["n"]) == [10, 11]
    full = {k: 0 for k in ["evaluation_time", "selection_time", "layout_time", "time", "normalized_influence", "influence",
                           "seed_method", "dim", "m", "n", "graph_type"]}
    assert list(gr.display_benchmark_results([full]).columns) == [
        "graph_type", "n", "m", "dim", "seed_method", "influence", "normalized_influence", "time", "layout_time",
        "selection_time", "evaluation_time"]


def test_plot_radial_vs_centrality():
    cols = grid_columns(50)
    names = ["Degree", "Betweenness", "Eigenvector", "PageRank"]
    fig = gr.plot_radial_vs_centrality(cols[0], [cols[1], cols[2], cols[6], cols[8]], names, show=False)
    facets = sorted(a.text.split("=")[-1] for a in fig.layout.annotations)
    assert facets == sorted(names)
    points = [t for t in fig.data if t.mode == "markers"]
    lines = [t for t in fig.data if t.mode == "lines"]
    assert len(points) == 4 and len(lines) == 4 and all(len(t.x) == 50 for t in points)
    # the line of a facet is the least-squares fit and sits on that facet's axes
    by_name = {t.name.replace(" fit", ""): t for t in lines}
    axes = {fig.data[i].xaxis for i in range(len(fig.data))}
    assert len(axes) == 4
    for name, y in zip(names, [cols[1], cols[2], cols[6], cols[8]]):
        slope, intercept = np.polyfit(cols[0], y, 1)
        line = by_name[name]
        assert np.allclose(line.y, slope * np.asarray(line.x) + intercept)
        scatter = next(t for t in points if np.array_equal(np.asarray(t.y, dtype=np.float64), y))
        assert scatter.xaxis == line.xaxis and scatter.yaxis == line.yaxis


def test_errors():
    good = np.arange(10, dtype=np.float64)
    for bad in (np.nan, np.inf, -np.inf):
        col = good.copy()
        col[4] = bad
        with pytest.raises(ValueError, match="non-finite"):
            _native.Correlation(np.stack([good, col]), -1)
    with pytest.raises(ValueError, match="at least 2"):
        _native.Correlation(np.zeros((2, 1)), -1)
    with pytest.raises(ValueError, match="128-bit"):
        _native.Correlation(np.zeros((1, 2097152)), -1)
    corr = _native.Correlation(np.stack([good, good[::-1]]), -1)
    for pair in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="column"):
            corr.bootstrap([pair], 4)
    for reps in (0, -3):
        with pytest.raises(ValueError, match="reps"):
            corr.bootstrap([[0, 1]], reps)
    with pytest.raises(ValueError, match="budget"):
        corr.set_memory_budget(-1)
    assert corr.bootstrap([[0, 1]], 3).tolist() == [[-1.0, -1.0, -1.0]]
    corr.close()
    with pytest.raises(ValueError, match="same length"):
        gr.spearman_matrix([good, good[:5]])


def test_accumulator_bound_on_the_host():
    n = 2097151
    x = np.arange(n, dtype=np.float64)
    corr = _native.Correlation(np.stack([x, -x]), -1)
    matrix, sums = corr.matrix(sums=True)
    corr.close()
    sxy, sxx, syy = (int(v) for v in sums[0, 1])
    assert sxx == syy == (n - 1) * n * (n + 1) // 3 and sxy == -sxx    # sum of (2k - (n - 1))^2, k = 0 .. n-1
    assert matrix[0, 1] == -1.0


def _fake_benchmark(monkeypatch):
    """benchmark_correlations over a run_benchmark that needs no GPU."""
    from graphem_rapids_amd import centrality
    cols = grid_columns(500)

    def run_benchmark(graph_generator, graph_params, **kwargs):
        out = {"n": 500, "radii": cols[0]}
        out.update(dict(zip(centrality.CORRELATION_KEYS, cols[[1, 2, 3, 5, 6, 8]])))
        return out
    monkeypatch.setattr(centrality, "run_benchmark", run_benchmark)
    return centrality, cols


def test_benchmark_correlations_keywords(monkeypatch):
    centrality, cols = _fake_benchmark(monkeypatch)
    plain = centrality.benchmark_correlations(gr.barabasi_albert_edges, dict(n=500, m=3))
    assert set(plain["correlations"]) == set(centrality.CORRELATION_KEYS)
    for name, col in zip(centrality.CORRELATION_KEYS, cols[[1, 2, 3, 5, 6, 8]]):
        assert set(plain["correlations"][name]) == {"rho", "p"}
        rho, p = stats.spearmanr(cols[0], col)
        assert same_bits(plain["correlations"][name]["rho"], rho) and same_bits(plain["correlations"][name]["p"], p)
    boot = centrality.benchmark_correlations(gr.barabasi_albert_edges, dict(n=500, m=3), bootstrap_reps=50, bootstrap_seed=4)
    _, _, lo, hi, _ = gr.bootstrap_spearman(cols[0], cols[[1, 2, 3, 5, 6, 8]], reps=50, seed=4)
    for j, name in enumerate(centrality.CORRELATION_KEYS):
        entry = boot["correlations"][name]
        assert set(entry) == {"rho", "p", "ci_low", "ci_high"}
        assert entry["ci_low"] <= entry["ci_high"]
        assert entry["ci_low"] == lo[j] and entry["ci_high"] == hi[j]
        assert same_bits(entry["rho"], plain["correlations"][name]["rho"])
