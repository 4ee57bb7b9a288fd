"""The sector-packed gather table of the three-component fused kernels (csrc/common.h gh_cg_slot, gh_phase_a<.., CG>,
plan.compact_gather): own rows and neighbour rows read from 12-byte rows packed five to a 64-byte sector hold the same
floats as the padded positions, so every step must leave the same bits with the switch ON and OFF -- also when the table
is out of date and the launch falls back to the padded form, and on engines whose plan cannot take it."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DEG, K_NN, S = 4099, 8, 10, 256   # 16 396 edges: just over the 16 384 the fused path needs; n no multiple of 5
HUB_DEG = 200                         # > GH_LONG_DEG (128): the hub's force comes from spring_long_kernel
STEPS = 5


@pytest.fixture(scope="module")
def graphs():
    import graphem_rapids_amd as gra
    rr = gra.random_regular_edges(N, DEG, seed=17).astype(np.int32)
    assert len(rr) == N * DEG // 2 == 16396
    rng = np.random.default_rng(5)
    spokes = np.stack([np.full(HUB_DEG, N), rng.permutation(N)[:HUB_DEG]], axis=1).astype(np.int32)
    return {"rr": (N, rr), "hub": (N + 1, np.vstack([rr, spokes]))}


def _inputs(n, D, E, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    stream = np.stack([rng.permutation(E)[:S] for _ in range(STEPS)]).astype(np.int32)
    return pos, stream


def _engine(n, D, edges, switch, form=None, **kw):
    from graphem_rapids_amd import _native
    eng = _native.Engine(n, D, edges, 1.0, 0.2, 0.5, K_NN, S, seed=3, **kw)
    if form is not None:
        eng.set_scan_filter(form)
        assert eng.scan_filter() == form
    eng.set_compact_gather(switch)
    return eng


def _five_steps(n, D, edges, switch, form, expect):
    pos, stream = _inputs(n, D, len(edges), 11)
    eng = _engine(n, D, edges, switch, form)
    assert eng.compact_gather() == expect
    eng.set_positions(pos)
    outs = []
    for t in range(STEPS):
        eng.step(stream[t])
        outs.append(eng.get_positions())
        assert eng.compact_gather() == expect
        assert eng.compact_gather_launches() == (t + 1 if expect else 0)   # what ran: the packed instantiation, every step
    eng.sync()
    eng.close()
    return outs


@pytest.mark.parametrize("form", ["cells", "mfma"])
@pytest.mark.parametrize("graph", ["rr", "hub"])
def test_five_steps_on_and_off_leave_the_same_bits(graph, form, graphs):
    n, edges = graphs[graph]
    on = _five_steps(n, 3, edges, "on", form, True)
    off = _five_steps(n, 3, edges, "off", form, False)
    for t in range(STEPS):
        assert on[t].tobytes() == off[t].tobytes(), f"step {t}"
    assert np.isfinite(on[-1]).all() and not np.array_equal(on[-1], on[0])


def _sequence(eng, n, E):
    """step, set_positions, step, the per-phase entry point, step, get_positions, step: every way the table can fall behind
    the positions between two fused launches."""
    pos, stream = _inputs(n, 3, E, 23)
    rng = np.random.default_rng(29)
    pos2 = (rng.standard_normal((n, 3)) * 0.2).astype(np.float32)
    Fs = (rng.standard_normal((n, 3)) * 0.01).astype(np.float32)
    Fi = (rng.standard_normal((n, 3)) * 0.01).astype(np.float32)
    outs, packed = [], []

    def ran():
        packed.append(eng.compact_gather_launches())
    eng.set_positions(pos)
    eng.step(stream[0]); ran()
    eng.set_positions(pos2)
    eng.step(stream[1]); ran()
    outs.append(eng.integrate_normalise(Fs, Fi))   # normalises into the position array and puts the positions back
    eng.step(stream[2]); ran()                      # the one step that must not read the table
    outs.append(eng.get_positions())
    eng.step(stream[3]); ran()
    eng.run(2); ran()                               # and the run loop with the engine's own draws behind it
    outs.append(eng.get_positions())
    eng.positions_device_ptr()                      # the rows are handed out: no launch reads the table from here on
    eng.step(stream[4]); ran()
    eng.set_positions(pos)
    eng.run(2); ran()
    outs.append(eng.get_positions())
    eng.sync()
    return outs, packed


@pytest.mark.parametrize("form", ["cells", "mfma"])
def test_a_table_that_fell_behind_is_not_read(form, graphs):
    n, edges = graphs["rr"]
    got = {}
    for switch in ("on", "off"):
        eng = _engine(n, 3, edges, switch, form)
        assert eng.compact_gather() == (switch == "on")
        got[switch] = _sequence(eng, n, len(edges))
        assert eng.compact_gather() is False   # (handed out at the end of the sequence)
        eng.close()
    for a, b in zip(got["on"][0], got["off"][0]):
        assert a.tobytes() == b.tobytes()
    # packed launches so far, after each stage: the step behind gh_integrate_normalise and everything behind
    # gh_positions_device ran the padded instantiation
    assert got["on"][1] == [1, 2, 2, 3, 5, 5, 5]
    assert got["off"][1] == [0] * 7


def test_switching_in_the_middle_of_a_run(graphs):
    """OFF -> ON allocates a table that holds nothing yet: the next launch must not read it."""
    n, edges = graphs["rr"]
    pos, stream = _inputs(n, 3, len(edges), 31)
    ref = _engine(n, 3, edges, "off", "cells")
    eng = _engine(n, 3, edges, "off", "cells")
    for e in (ref, eng):
        e.set_positions(pos)
        e.step(stream[0])
    eng.set_compact_gather("on")
    assert eng.compact_gather()
    for e in (ref, eng):
        e.step(stream[1])
        e.step(stream[2])
    assert eng.compact_gather_launches() == 1   # the first step behind the switch filled the table, the second read it
    eng.set_compact_gather("off")
    eng.set_compact_gather("on")
    for e in (ref, eng):
        e.step(stream[3])
    assert eng.compact_gather_launches() == 1 and ref.compact_gather_launches() == 0
    assert eng.get_positions().tobytes() == ref.get_positions().tobytes()
    ref.close()
    eng.close()


def test_split_f16_form_of_more_than_one_round_of_workgroups():
    """More than 2048 fused workgroups: the split-f16 kernel without its deferred pair list, the third packed instantiation."""
    import graphem_rapids_amd as gra
    n = 263000   # 1 052 000 edges in tiles of at most 512
    edges = gra.random_regular_edges(n, DEG, seed=19).astype(np.int32)
    pos, stream = _inputs(n, 3, len(edges), 41)
    outs = {}
    for switch in ("on", "off"):
        eng = _engine(n, 3, edges, switch, "mfma", reorder="off")
        eng.set_positions(pos)
        eng.step(stream[0])
        eng.step(stream[1])
        assert eng.compact_gather_launches() == (2 if switch == "on" else 0)
        outs[switch] = eng.get_positions()
        eng.close()
    assert outs["on"].tobytes() == outs["off"].tobytes()


@pytest.mark.parametrize("D", [2, 6])
def test_other_dimensions_leave_the_request_alone(D, graphs):
    n, edges = graphs["rr"]
    on = _five_steps(n, D, edges, "on", None, False)
    off = _five_steps(n, D, edges, "off", None, False)
    assert on[-1].tobytes() == off[-1].tobytes()


def test_a_two_rank_partition_leaves_the_request_alone(graphs):
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import partition_rows
    n, edges = graphs["rr"]
    pos, stream = _inputs(n, 3, len(edges), 37)
    lib = _native.load()
    world = 2
    outs = {}
    for switch in ("on", "off"):
        group = lib.gh_loopback_group_create(world)
        engines = []
        for r in range(world):
            chunk, lo, hi = partition_rows(n, world, r)
            e = _engine(n, 3, edges, switch, None, partition=(lo, hi, 0, 0, _native.EDGES_HASHED))
            e.overlap_layout(world, r, chunk)
            e.set_compact_gather(switch)   # (again, behind the layout)
            assert not e.compact_gather()
            e.comm_init_loopback(group, r)
            e.set_positions(pos)
            engines.append(e)
        errors = []

        def work(e):
            try:
                e.run_partitioned(3, stream[:3])
                e.sync()
            except Exception as exc:  # pylint: disable=broad-exception-caught
                errors.append(exc)
        threads = [threading.Thread(target=work, args=(e,)) for e in engines]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not errors and not any(t.is_alive() for t in threads), errors
        outs[switch] = [e.get_positions() for e in engines]
        for e in engines:
            assert not e.compact_gather()
            e.comm_destroy()
            e.close()
        lib.gh_loopback_group_destroy(group)
    assert outs["on"][0].tobytes() == outs["off"][0].tobytes()
    assert outs["on"][1].tobytes() == outs["on"][0].tobytes()
