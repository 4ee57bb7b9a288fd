"""Rank-correlation reports: the reference's visualization module (report_corr, report_full_correlation_matrix,
plot_radial_vs_centrality, display_benchmark_results) over the library's Spearman kernels.

spearman_matrix and bootstrap_spearman are the numpy-level interface everything else here uses.  They run on the device
when one is present and on the library's host path otherwise; both give the same numbers bit for bit
(include/graphem_hip.h "rank correlation").

The bootstrap stream is this package's own: resample b draws its n indices from the counter-based words
word(seed, b, j), so a report is a pure function of (data, reps, seed).  The reference draws from numpy's global state
(np.random.choice); the distribution is the same, the individual resamples are not, and numpy's global state is neither
read nor advanced here.

pandas and plotly are imported inside the functions that need them.
"""
import numpy as np

from . import _native

FULL_MATRIX_LABELS = ("Radius", "Degree", "Betweenness", "Eigenvector", "PageRank", "Closeness", "Node Load")
DISPLAY_COLUMNS = ("graph_type", "n", "m", "dim", "seed_method", "influence", "normalized_influence", "time",
                   "layout_time", "selection_time", "evaluation_time")


def _device_id(device_id=None):
    """The device the statistics run on: the given one, else device 0 when there is one, else -1 (the host path)."""
    if device_id is not None:
        return int(device_id)
    return 0 if _native.device_count() > 0 else -1


def _table(columns):
    rows = [np.asarray(c, dtype=np.float64).ravel() for c in columns]
    if not rows:
        raise ValueError("at least one column is needed")
    if any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("all columns must have the same length")
    return np.ascontiguousarray(np.stack(rows))


def spearman_p(rho, n):
    """Two-sided p-value of Spearman's rho over n points as scipy.stats.spearmanr computes it: Student's t with n - 2
    degrees of freedom at t = rho * sqrt((n - 2) / ((rho + 1) (1 - rho)))."""
    from scipy import special
    rho = np.asarray(rho, dtype=np.float64)
    dof = n - 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = rho * np.sqrt((dof / ((rho + 1.0) * (1.0 - rho))).clip(0))
    p = 2 * special.stdtr(dof, -np.abs(t))
    return p[()]


def spearman_matrix(columns, device_id=None):
    """(m, m) Spearman matrix of m equally long columns: symmetric, diagonal 1, NaN in the row and column of a constant
    column."""
    corr = _native.Correlation(_table(columns), _device_id(device_id))
    try:
        return corr.matrix()
    finally:
        corr.close()


def bootstrap_spearman(x, ys, reps=1000, seed=0, alpha=0.025, device_id=None):
    """Spearman's rho between x and every column of ys with a percentile bootstrap interval.

    Returns (rho, p, ci_low, ci_high, replicates): arrays of len(ys) -- rho of the data, its two-sided p, the
    100 alpha and 100 (1 - alpha) percentiles (np.percentile) of the replicates -- and the (len(ys), reps) replicate
    array.  One set of `reps` resamples (counter-based, see the module docstring) serves all columns."""
    ys = list(ys)
    table = _table([x] + ys)
    corr = _native.Correlation(table, _device_id(device_id))
    try:
        rho = corr.matrix()[0, 1:]
        pairs = np.array([[0, j + 1] for j in range(len(ys))], dtype=np.int32)
        replicates = corr.bootstrap(pairs, reps, seed)
    finally:
        corr.close()
    ci_low = np.percentile(replicates, 100 * alpha, axis=1)
    ci_high = np.percentile(replicates, 100 * (1 - alpha), axis=1)
    return rho, spearman_p(rho, table.shape[1]), ci_low, ci_high, replicates


def _report_line(name, rho, ci_low, ci_high, p):
    print(f"{name:15s}: rho = {rho:.3f} (95% CI: [{ci_low:.3f}, {ci_high:.3f}]), p = {p:.6f}")


def report_corr(name, radii, centrality, alpha=0.025, *, reps=1000, seed=0):
    """Prints Spearman's rho between the radii and one centrality with its bootstrap interval and p-value, in the
    reference's format, and returns (rho, p)."""
    rho, p, lo, hi, _ = bootstrap_spearman(radii, [centrality], reps=reps, seed=seed, alpha=alpha)
    _report_line(name, rho[0], lo[0], hi[0], p[0])
    return float(rho[0]), float(p[0])


def report_full_correlation_matrix(radii, deg, btw, eig, pr, clo, nload, alpha=0.025, *, reps=1000, seed=0):
    """Prints the correlation of the radii with each of the six centralities (as report_corr) and returns the 7 x 7
    Spearman matrix as a pandas DataFrame labelled like the reference's.  One handle over the seven columns, one
    bootstrap call for the six pairs."""
    import pandas as pd
    table = _table([radii, deg, btw, eig, pr, clo, nload])
    corr = _native.Correlation(table, _device_id())
    try:
        matrix = corr.matrix()
        pairs = np.array([[0, j] for j in range(1, 7)], dtype=np.int32)
        replicates = corr.bootstrap(pairs, reps, seed)
    finally:
        corr.close()
    rho = matrix[0, 1:]
    p = spearman_p(rho, table.shape[1])
    print("Correlations with radial distance:")
    for j, name in enumerate(FULL_MATRIX_LABELS[1:]):
        _report_line(name, rho[j], np.percentile(replicates[j], 100 * alpha), np.percentile(replicates[j], 100 * (1 - alpha)), p[j])
    return pd.DataFrame(matrix, index=list(FULL_MATRIX_LABELS), columns=list(FULL_MATRIX_LABELS))


def plot_radial_vs_centrality(radii, centralities, names, *, show=True):
    """Scatter plots of every centrality against the radial distance, one facet per name (three to a row), each with its
    least-squares line (fitted with numpy).  Returns the figure; show=True also displays it, as the reference does."""
    import pandas as pd
    import plotly.express as px
    radii = np.asarray(radii, dtype=np.float64).ravel()
    names = [str(name) for name in names]
    values = [np.asarray(c, dtype=np.float64).ravel() for c in centralities]
    if len(values) != len(names) or any(len(v) != len(radii) for v in values):
        raise ValueError("one centrality array of len(radii) per name is needed")
    frame = pd.DataFrame({"Radial Distance": np.tile(radii, len(names)),
                          "Centrality Value": np.concatenate(values) if values else np.zeros(0),
                          "Centrality Measure": np.repeat(names, len(radii))})
    fig = px.scatter(frame, x="Radial Distance", y="Centrality Value", facet_col="Centrality Measure", facet_col_wrap=3,
                     category_orders={"Centrality Measure": names},
                     title="Correlation between Radial Distance and Centrality Measures")
    wrap = min(3, max(1, len(names)))
    n_rows = (len(names) + wrap - 1) // wrap
    ends = np.array([radii.min(), radii.max()]) if len(radii) else np.zeros(2)
    for j, v in enumerate(values):
        if len(radii) >= 2 and ends[0] < ends[1]:
            slope, intercept = np.polyfit(radii, v, 1)
        else:
            slope, intercept = 0.0, float(v.mean()) if len(v) else 0.0
        # plotly numbers facet rows from the bottom
        fig.add_scatter(x=ends, y=slope * ends + intercept, mode="lines", name=f"{names[j]} fit", showlegend=False,
                        row=n_rows - j // wrap, col=j % wrap + 1)
    fig.update_layout(height=800, width=1000)
    if show:
        fig.show()
    return fig


def display_benchmark_results(benchmark_results):
    """The list of benchmark result dictionaries as a pandas DataFrame with the reference's columns, in its order;
    columns a result does not have are left out."""
    import pandas as pd
    frame = pd.DataFrame(benchmark_results)
    return frame[[col for col in DISPLAY_COLUMNS if col in frame.columns]]
