"""The box of a query ball in the cell frame of the query-cell pre-filter (csrc/qcell_core.h) is conservative: for every
(q, tau, m) whose fp32 distance chain -- the exact test of the fused kernel -- gives d2 <= tau, m's cell lies inside q's
box on every axis.  Checked on the library's host copy of the box and cell code (gh_qcell_probe); no GPU needed."""
import ctypes

import numpy as np
import pytest

G1 = 7   # boundaries per axis (GH_QC_G - 1)


def _probe(bounds, q, tau, m):
    from graphem_rapids_amd import _native
    lib = _native.load()
    n, D = q.shape
    bounds = np.ascontiguousarray(bounds, dtype=np.float32).reshape(D, G1)
    q, m = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(m, dtype=np.float32)
    tau = np.ascontiguousarray(tau, dtype=np.float32)
    d2 = np.empty(n, dtype=np.float32)
    cells = np.empty((n, D, 3), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gh_qcell_probe(p(bounds), D, p(q), p(tau), p(m), n, p(d2), p(cells)) == 0
    return d2, cells


def _near_sphere(rng, q, tau):
    """Midpoints on and just around the fp32 ball of radius sqrt(tau), nudged by a few ulps either way."""
    n, D = q.shape
    u = rng.standard_normal((n, D))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = np.sqrt(tau.astype(np.float64)) * (1.0 + rng.uniform(-1e-6, 1e-6, size=n))
    m = (q.astype(np.float64) + u * r[:, None]).astype(np.float32)
    steps = rng.integers(-3, 4, size=m.shape)
    out = m.copy()
    for s in range(1, 4):
        out = np.where(steps >= s, np.nextafter(out, np.float32(np.inf)), out)
        out = np.where(steps <= -s, np.nextafter(out, np.float32(-np.inf)), out)
    return out


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("scale", [1e-15, 1e-3, 1.0, 1e5])
def test_passing_midpoints_lie_inside_the_query_box(D, scale):
    rng = np.random.default_rng(100 + D)
    n = 40000
    q = (rng.standard_normal((n, D)) * scale).astype(np.float32)
    tau = (rng.uniform(0.0, 2.0, size=n) * scale * scale * rng.choice([1e-6, 1e-2, 1.0], size=n)).astype(np.float32)
    tau[::50] = 0.0   # collapsed layouts: tau = 0
    m = _near_sphere(rng, q, tau)
    m[::97] = q[::97]   # duplicates of the query itself
    # boundaries right where it is hardest: the coordinates of q and m themselves and their fp32 neighbours
    pool = np.concatenate([q.ravel(), m.ravel(), np.nextafter(m.ravel(), np.float32(np.inf)),
                           np.nextafter(m.ravel(), np.float32(-np.inf))])
    total, passing, narrow = 0, 0, 0
    for trial in range(8):
        idx = rng.integers(0, n, size=n)   # every triple with its own boundary set would be slow: 8 sets, reused
        b = np.sort(rng.choice(pool, size=D * G1, replace=False).reshape(D, G1), axis=1)
        if trial == 7:
            b = np.sort(q[idx[:G1]].T.astype(np.float32), axis=1)   # the boundaries ARE query coordinates
        d2, cells = _probe(b, q[idx], tau[idx], m[idx])
        ok = d2 <= tau[idx]
        c, lo, hi = cells[..., 0], cells[..., 1], cells[..., 2]
        inside = ((lo <= c) & (c <= hi)).all(axis=1)
        assert inside[ok].all(), f"a passing midpoint outside its query's box (trial {trial})"
        assert ((0 <= lo) & (lo <= hi) & (hi <= G1)).all()
        total += len(ok)
        passing += int(ok.sum())
        narrow += int(((hi - lo) <= 1).all(axis=1).sum())
    # the test has teeth: many triples pass, and most boxes are narrow
    assert 0.02 * total < passing < 0.9 * total
    assert narrow > 0.5 * total


def test_unsorted_and_nan_boundaries_stay_conservative():
    """The argument needs no order and no particular values: NaN boundaries (never <= anything) and unsorted ones."""
    rng = np.random.default_rng(7)
    n, D = 20000, 3
    q = rng.standard_normal((n, D)).astype(np.float32)
    tau = rng.uniform(0.0, 0.5, size=n).astype(np.float32)
    m = _near_sphere(rng, q, tau)
    b = rng.standard_normal((D, G1)).astype(np.float32)
    b[0, 3] = np.nan
    b[2, 0] = np.inf
    b[1, 6] = -np.inf
    d2, cells = _probe(b, q, tau, m)
    ok = d2 <= tau
    c, lo, hi = cells[..., 0], cells[..., 1], cells[..., 2]
    assert ok.sum() > n // 5
    assert ((lo <= c) & (c <= hi)).all(axis=1)[ok].all()
