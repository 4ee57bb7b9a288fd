"""What the float32 engine's intersection and update phases must give, stated so that float32 inputs have an essentially
exact answer: what tests/test_hip_f32_phases.py compares the kernels of csrc/forces.hip, csrc/intersect_core.h and the select
kernels with.  TEST INFRASTRUCTURE ONLY: plain numpy plus the `oracle` package, no GPU.  Anchored by
tests/test_f32_reference_cpu.py.

Update (pt.py:796-804).  new = fl32(pos + fl32(Fs + Fi)); the engine centres by mean32 = fl32(column mean of new) and divides
by sd32 = fl32(fl32(sqrt(unbiased variance of new)) + 1e-6f), mean and variance being EXACT functions of the float32 array
`new` (the kernels form them in double; here in long double, two-pass).  out = fl32(fl32(new - mean32) / sd32) is then
determined bit for bit except where the exact mean or standard deviation sits next to a float32 rounding boundary, so each
element has a bar that is derived, not measured:

    bar = (ulp(mean32) + ulp(new)) / sd32  +  |out| ulp(sd32) / sd32  +  ulp(out)

one ulp of the mean, one of `new` (the Fi of a whole step may differ from the per-phase call's in its last bit), one of the
standard deviation, one of the result.

Intersection (pt.py:638-774).  Every per-pair term is the oracle's float32 term (same operations, same order, no
contraction); only the summation differs -- the engine adds in double, the oracle in float32.  intersection_sum() has the
oracle produce every term UNSUMMED (each listed pair that passes the id rules gets four fresh vertices and two fresh edges
of its own, so every vertex of that call receives one term) and adds them in long double: the exact value of what the engine
accumulates.  Bar per element: ulp32(|exact|) + 2^-44 sum|terms| (the rounding of the sum to float32; up to 512 double
additions of 2^-53 relative each).
"""
import numpy as np

import f64_reference
import oracle
from f64_reference import LD, PLANTED_COUNTS, PLANTED_K, classify_planted, degree_ladder, scatter_add  # noqa: F401

F32 = np.float32
PRM = (1.0, 0.2, 0.5)     # L_min, k_attr, k_inter


def ulp32(x):
    """Distance from |x| (rounded to float32) to the next float32 above it, as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def integrate(pos, Fs, Fi):
    """fl32(pos + fl32(Fs + Fi)), pt.py:796-799."""
    pos, Fs, Fi = (np.asarray(a, dtype=F32) for a in (pos, Fs, Fi))
    return pos + (Fs + Fi)


def exact_stats(new):
    """(mean, unbiased variance) of the columns of a float32 array, in long double, two-pass."""
    x = np.asarray(new, dtype=LD)
    n = x.shape[0]
    mean = x.sum(axis=0) / LD(n)
    c = x - mean
    return mean, (c * c).sum(axis=0) / LD(n - 1)


def _finish(new, snew):
    mean, var = exact_stats(snew)
    mean32 = mean.astype(F32)
    sd32 = np.sqrt(var).astype(F32) + F32(1e-6)
    assert mean32.dtype == F32 and sd32.dtype == F32
    out = (new - mean32) / sd32
    assert out.dtype == F32
    sd = sd32.astype(np.float64)
    bar = (ulp32(mean32) + ulp32(new)) / sd + np.abs(out.astype(np.float64)) * ulp32(sd32) / sd + ulp32(out)
    return out, bar


def update(pos, Fs, Fi):
    """(out float32, bar float64), both (n, D): see the module docstring."""
    new = integrate(pos, Fs, Fi)
    return _finish(new, new)


def update_stats_from(pos, Fs, Fi, Fi_for_stats):
    """update(), but mean and standard deviation are those of pos + (Fs + Fi_for_stats): what an engine would give that
    integrated the right rows and took its statistics from others.  Only used to state a condition on inputs (a lost
    correction must lie many bars from the right answer)."""
    return _finish(integrate(pos, Fs, Fi), integrate(pos, Fs, Fi_for_stats))


def one_pass_model(new, n=None):
    """A numpy model of the kernels' statistics (normalise_kernel): float64 sums of x and x * x, mean = sum / n,
    var = max((sq - sum * mean) / (n - 1), 0), mean32 = (float)mean, sd32 = (float)sqrt(var) + 1e-6f; then the same two
    float32 operations per element.  (numpy adds pairwise, the kernels by workgroup: both are sums of doubles.)"""
    new = np.asarray(new, dtype=F32)
    n = new.shape[0] if n is None else n
    x = new.astype(np.float64)
    s, sq = x.sum(axis=0), (x * x).sum(axis=0)
    m = s / float(n)
    var = np.maximum((sq - s * m) / float(n - 1), 0.0)
    return (new - m.astype(F32)) / (np.sqrt(var).astype(F32) + F32(1e-6))


def fraction(got, ref, bar):
    """Worst |got - ref| / bar over the array (0 where both are equal, bar or no bar)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bar)
    return float(f.max()) if f.size else 0.0


# ---- intersection ---------------------------------------------------------------------------------------------------

def unrolled_terms(pos, edges, sampled, knn, k_inter=PRM[2]):
    """(ends (P, 4) vertex ids, terms (P, 4, D) float32, i (P,), j (P,)) for the P listed pairs (i, j) that pass the id
    rules (i < j, no shared vertex; a pair listed twice is there twice).  terms[p, r] is the oracle's float32 force on
    endpoint r (p1, p2, q1, q2) of pair p -- zeros for a pair that does not cross -- produced by ONE call of
    oracle.intersection_forces on 4 P fresh vertices and 2 P fresh edges, sampled = [2 p], knn = [[2 p + 1]], k = 1."""
    pos = np.ascontiguousarray(pos, dtype=F32)
    edges = np.asarray(edges, dtype=np.int64)
    knn = np.asarray(knn, dtype=np.int64)
    D = pos.shape[1]
    i = np.repeat(np.asarray(sampled, dtype=np.int64), knn.shape[1])
    j = knn.reshape(-1)
    keep = i < j
    i, j = i[keep], j[keep]
    e1, e2 = edges[i], edges[j]
    share = (e1[:, 0] == e2[:, 0]) | (e1[:, 0] == e2[:, 1]) | (e1[:, 1] == e2[:, 0]) | (e1[:, 1] == e2[:, 1])
    i, j = i[~share], j[~share]
    ends = np.concatenate([edges[i], edges[j]], axis=1)          # (P, 4)
    P = len(i)
    if P == 0 or D < 2:
        return ends, np.zeros((P, 4, D), dtype=F32), i, j
    fresh_pos = np.ascontiguousarray(pos[ends.reshape(-1)])      # vertex 4 p + r carries the row of ends[p, r]
    fresh_edges = np.arange(4 * P, dtype=np.int32).reshape(2 * P, 2)
    terms = oracle.intersection_forces(fresh_pos, fresh_edges, 2 * np.arange(P, dtype=np.int32),
                                       (2 * np.arange(P, dtype=np.int32) + 1).reshape(P, 1), k_inter)
    return ends, terms.reshape(P, 4, D), i, j


def intersection_sum(pos, edges, sampled, knn, k_inter=PRM[2]):
    """(exact (n, D) long double, sum_abs (n, D) long double, touched (n,) bool): the unsummed terms of unrolled_terms
    scatter-added onto the original vertices in long double; their absolute values likewise; the vertices of crossing
    pairs.  D < 2: zeros, nothing touched (the crossing test needs coordinates 0 and 1)."""
    pos = np.asarray(pos, dtype=F32)
    n, D = pos.shape
    ends, terms, _, _ = unrolled_terms(pos, edges, sampled, knn, k_inter)
    crossing = terms.reshape(len(ends), -1).any(axis=1)
    idx = ends[crossing].reshape(-1)
    vals = terms[crossing].reshape(-1, D).astype(LD)
    touched = np.zeros(n, dtype=bool)
    touched[idx] = True
    return scatter_add(n, idx, vals), scatter_add(n, idx, np.abs(vals)), touched


def intersection_bar(exact, sum_abs):
    return ulp32(exact) + 2.0 ** -44 * np.asarray(sum_abs, dtype=np.float64)


def crossing_count(pos, edges, sampled, knn):
    _, terms, _, _ = unrolled_terms(pos, edges, sampled, knn)
    return int(terms.reshape(len(terms), -1).any(axis=1).sum())


# ---- inputs shared by the CPU anchor and the GPU tests --------------------------------------------------------------

PLANTED_DIMS = tuple(range(2, 17)) + (17, 20, 40, 1)


def planted(D):
    """f64_reference.planted_intersections with float32 positions (coordinates 0 and 1 are small integers: exact)."""
    pos, edges, sampled, knn, hub = f64_reference.planted_intersections(D)
    return pos.astype(F32), edges, sampled, knn, hub


STARTS = ("gauss", "scaled_1e-4", "scaled_1e4", "shift_1000", "shift_1e5", "constant")


def start_state(kind, n, D, seed):
    """A float32 start of the update tests: Gaussian; scaled by 1e-4 and 1e4; column 0 shifted by 1000 and by 1e5; the last
    column constant (2.5)."""
    pos = np.random.default_rng(seed).standard_normal((n, D))
    if kind == "scaled_1e-4":
        pos *= 1e-4
    elif kind == "scaled_1e4":
        pos *= 1e4
    elif kind == "shift_1000":
        pos[:, 0] += 1000.0
    elif kind == "shift_1e5":
        pos[:, 0] += 1e5
    elif kind == "constant":
        pos[:, D - 1] = 2.5
    elif kind != "gauss":
        raise ValueError(kind)
    return pos.astype(F32)


def injected_forces(pos, seed):
    """(Fs, Fi) for integrate_normalise alone: Fs Gaussian at 0.05 of the cloud's scale, zero in a constant column (a
    constant column has no spring force); Fi zero except on 5 % of the rows (at least one), where it is fifty times that."""
    n, D = pos.shape
    rng = np.random.default_rng(seed)
    scale = np.maximum(np.asarray(pos, dtype=np.float64).std(axis=0), 0.0)
    scale = np.where(scale > 0, scale, 0.0)
    Fs = rng.standard_normal((n, D)) * 0.05 * scale
    Fi = np.zeros((n, D))
    rows = rng.permutation(n)[: max(1, n // 20)]
    Fi[rows] = rng.standard_normal((len(rows), D)) * 2.5 * scale
    return Fs.astype(F32), Fi.astype(F32)


# n, D of integrate_normalise alone.  Row stride LD = 4 (D <= 4), 8 (D <= 8), 16 (D <= 16), else D rounded up to 4; the
# normalise grid is ceil(n LD / 4 / 1024) workgroups capped at 2048 (gh_launch_normalise), i.e. capped from n LD > 8 388 608;
# column_stats_kernel strides rows by 256.
UPDATE_SHAPES = [(2, 3), (3, 5), (2, 17), (255, 1), (257, 4), (1000, 9), (4099, 33), (20001, 3), (20001, 8), (20001, 16),
                 (20001, 17), (2097151, 3), (2097153, 4), (1048577, 5), (524289, 9), (233011, 33), (233017, 33)]
UPDATE_CASES = [(n, D, s) for n, D in UPDATE_SHAPES for s in (STARTS if (n, D) in ((20001, 3), (20001, 8), (20001, 16), (20001, 17)) else ("gauss", "shift_1000"))]


def row_stride(D):
    return 4 if D <= 4 else 8 if D <= 8 else 16 if D <= 16 else 4 * ((D + 3) // 4)


def hub_graph():
    """The graph of test_hip_parity.test_skewed_degrees_hubs: hubs of degree 20000, 2000 and 600 on a 4-regular graph of
    50000 vertices (one row owns more edges than a fused workgroup holds: the unfused kernels, the long-row kernels)."""
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
    return n, np.ascontiguousarray(e, dtype=np.int32)


def regular_graph(n, deg, seed):
    import graphem_rapids_amd as gra
    return np.ascontiguousarray(gra.random_regular_edges(n, deg, seed=seed), dtype=np.int32)


# The update inside step() with sample_size = 0: name -> (graph, D).  A step that samples nothing never runs the fused
# spring+scan kernel (step_begin_launches sends it to gh_launch_spring_mid whatever the number of edges), so new0 is never
# ready and gh_launch_integrate always takes integrate_kernel<LD> + stats_reduce_kernel (LD = 4, 8, 16) or
# integrate_generic_kernel + column_stats_kernel (D > 16): stats_fix_kernel cannot be reached this way and is covered by the
# whole-step cases below.  "many*": 70000 rows = 274 workgroups of integrate_kernel, so stats_reduce_kernel's 256 threads take
# a second trip over the partials; the hub graph and the degree ladder feed the update from the long-row spring kernels.
NOSAMPLE_CASES = {
    "unfused4": ("rr3000", 3), "unfused8": ("rr3000", 6), "unfused16": ("rr3000", 12), "general": ("rr3000", 20),
    "many4": ("rr70000", 3), "many8": ("rr70000", 8), "many16": ("rr70000", 16), "hubs": ("hubs", 3), "ladder": ("ladder", 8),
}


def nosample_graph(name):
    g = NOSAMPLE_CASES[name][0]
    if g == "hubs":
        return hub_graph()
    if g == "ladder":
        return degree_ladder()
    n = int(g[2:])
    return n, regular_graph(n, 4 if n < 4000 else 8, seed=n)


# A whole step with the intersection phase: name -> n, D, degree (0: the hub graph), k, S, engine keywords, rows ("exact":
# oracle.knn_midpoints, "aten": oracle.knn_midpoints_aten), and the kernel that runs the pairs.  intersect_query
# (select_core.h) takes gh_intersect_query_wide for every D in 2..16 with k <= 127, gh_intersect_pair_t for those D with
# k >= 128 and gh_intersect_pair for D > 16; a single-rank engine with k + 1 > 128 does not run the pairs in its select launch
# at all (intersect_kernel afterwards), so gh_intersect_pair_t inside intersect_query is reached only through the merge kernel
# of a partitioned step: PARTITION_CASES["sort"].  stats_fix_kernel<4, 8, 16> runs with skip_reduce = 1 in the fused cases
# with S < 2048 (fused, wide8, wide16) and reduces by itself from S = 2048 on (wave, wave8, wave16).
# The grid search exists for D <= 3 only (gh_grid_path; knn_method="grid" at D = 6 would run the scan): no grid case at D = 6.
STEP_CASES = {
    "per_query": dict(n=3000, D=5, deg=4, k=10, S=256, kw={}, rows="exact"),           # knn_block_select_kernel, gh_intersect_query_wide<5, 8>
    "per_query_general": dict(n=2000, D=20, deg=4, k=10, S=256, kw={}, rows="exact"),  # the same kernel, gh_intersect_pair (scratch)
    "scan4_unfused": dict(n=50000, D=3, deg=0, k=10, S=1024, kw=dict(reorder="off"), rows="exact"),   # knn_select_kernel, wide, LD 4
    "wide8": dict(n=12000, D=8, deg=8, k=12, S=512, kw={}, rows="exact"),              # gh_intersect_query_wide<8, 8>
    "wide16": dict(n=10000, D=16, deg=8, k=32, S=256, kw={}, rows="exact"),            # gh_intersect_query_wide<16, 16>
    "sort": dict(n=20000, D=3, deg=8, k=130, S=64, kw={}, rows="exact"),               # knn_block_select_sort_kernel selects; pairs: intersect_kernel<3>
    "fused": dict(n=20000, D=3, deg=8, k=10, S=1024, kw={}, rows="exact"),             # fused spring+scan, stats_fix with skip_reduce
    "wave": dict(n=20000, D=3, deg=8, k=10, S=2048, kw={}, rows="exact"),              # knn_select_wave_kernel, stats_fix reduces itself
    "wave8": dict(n=12000, D=8, deg=8, k=12, S=2048, kw={}, rows="exact"),             # the same, stats_fix_kernel<8>, skip_reduce = 0
    "wave16": dict(n=10000, D=16, deg=8, k=32, S=2048, kw={}, rows="exact"),           # the same, stats_fix_kernel<16>, skip_reduce = 0
    "cdist": dict(n=20000, D=3, deg=8, k=10, S=1024, kw=dict(knn_distance="cdist"), rows="aten"),     # knn_select_cdist_kernel
    "grid3": dict(n=20000, D=3, deg=8, k=10, S=1024, kw=dict(knn_method="grid"), rows="exact"),
    "ivf3": dict(n=20000, D=3, deg=8, k=10, S=1024, kw=dict(knn_method="ivf", ivf_probes=-1), rows="exact"),
    "ivf6": dict(n=20000, D=6, deg=8, k=10, S=1024, kw=dict(knn_method="ivf", ivf_probes=-1), rows="exact"),
}
# states of STEP_CASES at D = 3 and D = 8 -> world sizes; "sort" (k = 130): knn_merge_kernel -> gh_intersect_pair_t<3, 4>
PARTITION_CASES = {"fused": (2, 3, 5), "wide8": (2, 3, 5), "sort": (2,)}


def step_case(name):
    """(n, D, edges, pos, k, S, samples (2, S), engine keywords, rows function)."""
    c = STEP_CASES[name]
    n, D = c["n"], c["D"]
    if c["deg"] == 0:
        n, edges = hub_graph()
    else:
        edges = regular_graph(n, c["deg"], seed=n + D)
    rng = np.random.default_rng(500 + n + D)
    pos = rng.standard_normal((n, D)).astype(F32)
    samples = np.stack([rng.permutation(len(edges))[: c["S"]] for _ in range(2)]).astype(np.int32)
    rows = oracle.knn_midpoints if c["rows"] == "exact" else oracle.knn_midpoints_aten
    return n, D, edges, pos, c["k"], c["S"], samples, c["kw"], rows


def step_conditions(pos, edges, sampled, knn, Fs):
    """The conditions a whole-step input must meet, from the oracle and the restatement alone: (crossing pairs, fraction of
    vertices touched, how many bars update_stats_from(..., Fi_for_stats = 0) lies from update(...) at its farthest
    element), and (Fi float32, out, bar) for the caller."""
    exact, _, touched = intersection_sum(pos, edges, sampled, knn)
    Fi = exact.astype(F32)
    out, bar = update(pos, Fs, Fi)
    lost, _ = update_stats_from(pos, Fs, Fi, np.zeros_like(Fi))
    return (crossing_count(pos, edges, sampled, knn), float(touched.mean()), fraction(lost, out, bar)), (Fi, out, bar)


def assert_step_conditions(cond, what=""):
    crossing, touched, lost = cond
    assert crossing >= 200, (what, cond)
    assert touched >= 0.05, (what, cond)
    assert lost > 10.0, (what, cond)
