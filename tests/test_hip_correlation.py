"""gh_corr_* (csrc/correlation.hip) on the device: against the restatement of the header's rules
(tests/correlation_reference.py) bit for bit on the CPU grid, against the library's host path at a million points,
against itself (memory budgets, a second run), at the accumulator bound, and end to end behind run_benchmark."""
import numpy as np
import pytest

import graphem_rapids_amd as gr
from graphem_rapids_amd import _native
from test_correlation_cpu import GRID_N, check_against_restatement

pytestmark = pytest.mark.gpu

STAR = [[0, j] for j in range(1, 7)]


def realistic_columns(n):
    """Seven columns shaped like a benchmark's: continuous radii, integer degrees with heavy ties, a column that is zero
    for most points (betweenness on a tree's leaves), and four more continuous or tied ones."""
    rng = np.random.default_rng(77)
    degree = np.floor(rng.pareto(2.0, n) * 2 + 1)
    radii = 5.0 / np.sqrt(degree) + rng.standard_normal(n) * 0.3
    btw = np.where(rng.random(n) < 0.8, 0.0, rng.random(n) * degree)
    eig = np.exp(rng.standard_normal(n)) * degree
    pr = degree / degree.sum() + rng.random(n) * 1e-9
    clo = np.round(0.2 + rng.standard_normal(n) * 0.01, 4)
    load = btw * 1.5 + np.where(btw > 0, rng.random(n), 0.0)
    return np.stack([radii, degree, btw, eig, pr, clo, load])


@pytest.mark.parametrize("n", GRID_N)
def test_device_equals_restatement(n):
    check_against_restatement(0, n)


@pytest.fixture(scope="module")
def million():
    cols = realistic_columns(1_000_000)
    host = _native.Correlation(cols, -1)
    want = host.bootstrap(STAR, 64, 3, sums=True), host.matrix(sums=True)
    host.close()
    device = _native.Correlation(cols, 0)
    yield device, want
    device.close()


def test_device_equals_host_at_a_million(million):
    device, ((want_rho, want_sums), (want_matrix, want_matrix_sums)) = million
    rho, sums = device.bootstrap(STAR, 64, 3, sums=True)
    assert np.array_equal(sums, want_sums)
    assert np.array_equal(rho.view(np.uint64), want_rho.view(np.uint64))
    assert np.isfinite(rho).all() and len(np.unique(rho[0])) == 64
    matrix, matrix_sums = device.matrix(sums=True)
    assert np.array_equal(matrix_sums, want_matrix_sums)
    assert np.array_equal(matrix.view(np.uint64), want_matrix.view(np.uint64))
    assert matrix.shape == (7, 7) and np.all(np.diag(matrix) == 1.0)


def test_memory_budget_and_rerun_do_not_change_results(million):
    device, ((want_rho, want_sums), _) = million
    # one replicate per batch, 17 per batch, everything at once, the default (and with it a second run of each)
    for budget in (1, 1 << 30, 64 << 30, 0, 1 << 30):
        device.set_memory_budget(budget)
        rho, sums = device.bootstrap(STAR, 64, 3, sums=True)
        assert np.array_equal(sums, want_sums), budget
        assert np.array_equal(rho.view(np.uint64), want_rho.view(np.uint64)), budget
    device.set_memory_budget(0)


def test_accumulator_bound():
    n = 2097151
    x = np.arange(n, dtype=np.float64)
    device = _native.Correlation(np.stack([x, -x]), 0)
    matrix, sums = device.matrix(sums=True)
    rho, rep_sums = device.bootstrap([[0, 1]], 2, 1, sums=True)
    device.close()
    sxy, sxx, syy = (int(v) for v in sums[0, 1])
    assert sxx == syy == (n - 1) * n * (n + 1) // 3 and sxy == -sxx
    assert matrix[0, 1] == -1.0
    assert np.all(rep_sums[..., 0] == -rep_sums[..., 1]) and np.all(rep_sums[..., 1] == rep_sums[..., 2])
    assert np.all(rho == -1.0)


def test_end_to_end_behind_run_benchmark(capsys):
    import pandas as pd
    res = gr.run_benchmark(gr.barabasi_albert_edges, dict(n=20000, m=3))
    columns = [res[k] for k in ("radii", "degree", "betweenness", "eigenvector", "pagerank", "closeness", "node_load")]
    frame = gr.report_full_correlation_matrix(*columns, reps=100)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 7 and out[1].startswith("Degree         : rho = ")
    theirs = pd.DataFrame(dict(zip(frame.columns, columns))).corr(method="spearman").to_numpy()
    assert frame.shape == (7, 7) and np.abs(frame.to_numpy() - theirs).max() <= 8 * 20000 * 2.0 ** -53
    host = gr.spearman_matrix(columns, device_id=-1)
    assert np.array_equal(frame.to_numpy().view(np.uint64), host.view(np.uint64))
