"""The rows of the next iteration's KNN set-up, gathered once by workgroups appended to the stats_fix launch
(csrc/setup_core.h gh_setup_gather) and read from that buffer by the set-up workgroups of the normalise launch behind it.

The staged path must give the bits of the stand-alone set-up (knn_setup_kernel on the finished positions), which an engine
created under GRAPHEM_HIP_NO_PRESETUP=1 runs in every iteration.  The graph is the one test_hip_dimension_sweep.py uses for
the fused path: random regular, 4200 vertices of degree 8 = 16 800 edges, just over GH_SCAN_MIN_EDGES.

A run stages rows for an iteration whose ids it can name before its stats_fix launch: the next row of a given stream, or
the engine's own draw (device sampler, arange).  So the device-sampler engines advance by run(1) -- every call stages the
next draw -- and the given-id engines run the first t rows of one stream from the same start for t = 1..6, which is the
state after each of the six iterations.  Needs a real MI355X (`pytest -m gpu`)."""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, DEG, K = 4200, 8, 10
PARAMS = (1.0, 0.2, 0.5)   # L_min, k_attr, k_inter
ITERS = 6
TOUCHED_SEED = 0           # see test_touched_endpoints


@functools.lru_cache(maxsize=None)
def _edges():
    import graphem_rapids_amd as gra
    edges = np.ascontiguousarray(gra.random_regular_edges(N, DEG, seed=N), dtype=np.int32)
    edges.setflags(write=False)
    return edges


@functools.lru_cache(maxsize=None)
def _start(D, seed=0, flat=False):
    pos = np.random.default_rng(100 * D + seed).standard_normal((N, D)).astype(np.float32)
    if flat:   # nearly planar: many edge crossings, so the intersection phase touches many rows
        pos[:, 2:] *= np.float32(1e-3)
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def _stream(S, iters=ITERS, seed=0):
    E = len(_edges())
    rng = np.random.default_rng(7000 + 10 * S + seed)
    ids = np.stack([rng.permutation(E)[:S] for _ in range(iters)]).astype(np.int32)
    ids.setflags(write=False)
    return ids


def _engine(D, S):
    from graphem_rapids_amd import _native
    return _native.Engine(N, D, _edges(), *PARAMS, K, S)


def _states(D, S, sampler, start):
    """Positions after each of ITERS iterations from `start` (see the module docstring)."""
    eng = _engine(D, S)
    out = []
    try:
        if sampler == "device":
            eng.set_positions(start)
            for _ in range(ITERS):
                eng.run(1)
                out.append(eng.get_positions())
        else:
            ids = _stream(S)
            for t in range(1, ITERS + 1):
                eng.set_positions(start)
                eng.run(t, ids[:t])
                out.append(eng.get_positions())
    finally:
        eng.close()
    return out


def _assert_same_states(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(b).all(), (what, t)
        assert np.array_equal(a, b), f"{what}: positions differ after iteration {t + 1}"


@pytest.mark.parametrize("sampler", ["device", "given"])
@pytest.mark.parametrize("S", [256, 300, 1024])   # 300: a partial second round of the set-up's query loop
@pytest.mark.parametrize("D", [2, 3, 6, 12])      # row strides 4, 4, 8, 16
def test_staged_equals_standalone_setup(D, S, sampler, monkeypatch):
    staged = _states(D, S, sampler, _start(D))
    monkeypatch.setenv("GRAPHEM_HIP_NO_PRESETUP", "1")
    alone = _states(D, S, sampler, _start(D))
    _assert_same_states(staged, alone, f"D={D} S={S} {sampler}")


def test_all_edges_sampled(monkeypatch):
    """sample_size >= E: the ids are arange(E), named by the engine itself."""
    E = len(_edges())
    staged = _states(3, E, "device", _start(3))
    monkeypatch.setenv("GRAPHEM_HIP_NO_PRESETUP", "1")
    alone = _states(3, E, "device", _start(3))
    _assert_same_states(staged, alone, "S = E")


@pytest.mark.parametrize("D,S", [(3, 256), (6, 300)])
def test_run_equals_steps(D, S):
    """run(6) stages the rows of iterations 2..6 (and of the draw after them); six step() calls each stage the next draw."""
    a, b = _engine(D, S), _engine(D, S)
    try:
        a.set_positions(_start(D))
        b.set_positions(_start(D))
        a.run(ITERS)
        for _ in range(ITERS):
            b.step()
        assert np.array_equal(a.get_positions(), b.get_positions())
    finally:
        a.close()
        b.close()


@functools.lru_cache(maxsize=None)
def _touched_overlap(seed):
    """The oracle's own run from the flat start: per iteration t, how many endpoints of iteration t + 1's queries the
    intersection phase of iteration t touched (rows with a non-zero intersection force)."""
    edges, ids = _edges(), _stream(256, ITERS, seed)
    pos = np.array(_start(3, seed, flat=True))
    overlap = []
    for t in range(ITERS - 1):
        knn = oracle.knn_midpoints(pos, edges, ids[t], K)
        Fi = oracle.intersection_forces(pos, edges, ids[t], knn, PARAMS[2])
        touched = np.nonzero(np.any(Fi != 0, axis=1))[0]
        nxt = np.unique(edges[ids[t + 1]].ravel())
        overlap.append(int(np.intersect1d(touched, nxt).size))
        pos = oracle.step(pos, edges, ids[t], K, *PARAMS)
    return overlap


def test_touched_endpoints(monkeypatch):
    """Query endpoints the intersection phase has just moved: their rows are recomputed from pos, Fs and the accumulators
    (stats_fix_kernel's expression), not read from the buffer the same launch is correcting.  TOUCHED_SEED was picked on
    the CPU: with it the oracle's run has such endpoints (seed 0: 239, 253, 235, 223, 205 of the 512 in iterations 1..5)."""
    overlap = _touched_overlap(TOUCHED_SEED)
    assert max(overlap) >= 1, overlap
    from graphem_rapids_amd import _native
    ids, start = _stream(256, ITERS, TOUCHED_SEED), _start(3, TOUCHED_SEED, flat=True)

    def states():
        eng = _native.Engine(N, 3, _edges(), *PARAMS, K, 256)
        out = []
        try:
            for t in range(1, ITERS + 1):
                eng.set_positions(start)
                eng.run(t, ids[:t])
                out.append(eng.get_positions())
        finally:
            eng.close()
        return out
    staged = states()
    monkeypatch.setenv("GRAPHEM_HIP_NO_PRESETUP", "1")
    _assert_same_states(staged, states(), "touched endpoints")


@pytest.mark.parametrize("flip", [False, True])
def test_invalidation(flip):
    """A set-up done ahead for the engine's own draw, then another start and other ids: the stand-alone set-up runs.
    flip: the scan filter changes in between as well (another threshold placement)."""
    D, S = 3, 256
    ids = _stream(S)[:2]
    p = _start(D, seed=1)
    eng, fresh = _engine(D, S), _engine(D, S)
    try:
        eng.set_positions(_start(D))
        eng.run(2)   # leaves the set-up of its next draw behind
        if flip:
            eng.set_scan_filter("mfma" if eng.scan_filter() == "cells" else "cells")
            fresh.set_scan_filter(eng.scan_filter())
        eng.set_positions(p)
        eng.run(2, ids)
        fresh.set_positions(p)
        fresh.run(2, ids)
        assert np.array_equal(eng.get_positions(), fresh.get_positions())
    finally:
        eng.close()
        fresh.close()


def test_staged_path_ran():
    """From the second iteration of a run on, no stand-alone set-up is launched; the two launches that share the set-up are."""
    eng = _engine(3, 256)
    try:
        eng.set_positions(_start(3))
        eng.run(1)
        eng.timing_enable(True)
        eng.timing_reset()
        eng.run(3)
        eng.sync()
        names = eng.timings()
        eng.timing_enable(False)
        assert "knn_setup" not in names, sorted(names)
        assert names["stats_fix"][1] == 3 and names["normalise"][1] == 3, names
    finally:
        eng.close()
