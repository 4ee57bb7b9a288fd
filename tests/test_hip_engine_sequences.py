"""History must not show: what a call on a float32 engine returns, or leaves in the positions, depends on the engine's
configuration, the current positions, the iteration counter and the call's arguments -- and on nothing else the handle has
done (a set-up made ahead, the flags of an unfinished step, a table copy filled and never consumed, buffers a previous
launch was to clean, counters and rings that outlive a call).

tests/engine_sequences.py has the operations, the seeded generator, the hand-written sequences and the replay model, which
runs every operation on a fresh engine started from the positions the model holds.  Every comparison is bit for bit.  The
model's pass comes first, so that the calls on the engine under test go out back to back: nothing synchronises between
them but what the sequence itself holds.  Needs a real MI355X (`pytest -m gpu`)."""
import functools

import numpy as np
import pytest

import engine_sequences as es
import sampler_reference

pytestmark = pytest.mark.gpu

ENV_SWITCHES = ("GRAPHEM_HIP_TAU_SEPARATE", "GRAPHEM_HIP_COARSE_TAU", "GRAPHEM_HIP_NO_PRESETUP", "GRAPHEM_HIP_REORDER")


@functools.lru_cache(maxsize=None)
def _edges(n):
    import graphem_rapids_amd as gra
    edges = np.ascontiguousarray(gra.random_regular_edges(n, es.DEGREE, seed=n), dtype=np.int32)
    edges.setflags(write=False)
    assert len(edges) == n * es.DEGREE // 2
    return edges


@pytest.fixture
def make_engine(monkeypatch):
    """cfg -> an engine of the configuration as it is right after creation.  The switches an engine reads from the
    environment when it is created are set for that creation only."""
    from graphem_rapids_amd import _native

    def make(cfg):
        with monkeypatch.context() as m:
            for name in ENV_SWITCHES:
                m.delenv(name, raising=False)
            for name, value in cfg.env.items():
                m.setenv(name, value)
            eng = _native.Engine(cfg.n, cfg.D, _edges(cfg.n), *es.PARAMS, cfg.k, cfg.samples, seed=es.ENGINE_SEED, **cfg.kw)
        if cfg.coarse:
            eng.set_coarse_tau(cfg.coarse)
        return eng
    return make


def _named(names, want):
    return any(nm.startswith(want[:-1]) if want.endswith("*") else nm == want for nm in names)


@pytest.mark.parametrize("name", list(es.CONFIGS))
def test_configuration_is_what_its_name_says(name, make_engine):
    """Once per configuration: the pre-filter and threshold form the engine reports, and the phases of one timed step.
    A threshold of csrc/step_plan.h that moves fails here, not by the sequences silently testing another path."""
    cfg = es.CONFIGS[name]
    eng = make_engine(cfg)
    try:
        assert (eng.n, eng.D, eng.E, eng.S, eng.k) == (cfg.n, cfg.D, cfg.E, cfg.samples, cfg.k)
        if es.REPORTS[name] is not None:
            assert (eng.scan_filter(), eng.coarse_tau()) == es.REPORTS[name]
        if name == "fused_wide":
            assert eng.ld == 8
        if not cfg.filter_ops:
            if cfg.D > 3 or cfg.samples > 256:
                with pytest.raises(ValueError):
                    eng.set_scan_filter("cells")
        else:
            eng.set_scan_filter("cells")
            eng.set_scan_filter("auto")
        eng.set_positions(es.cloud_of(cfg, 0))
        eng.timing_enable(True)
        eng.timing_reset()
        eng.step(es.ids_of(cfg, 0))
        names = sorted(eng.timings())
        eng.timing_enable(False)
        for want in cfg.expect:
            assert _named(names, want), (want, names)
        for unwanted in cfg.absent:
            assert not _named(names, unwanted), (unwanted, names)
        if cfg.queries and name != "block":   # a second step of a run: the set-up rides in the normalise launch
            eng.timing_enable(True)
            eng.timing_reset()
            eng.run(2)
            names = eng.timings()
            eng.timing_enable(False)
            assert names.get("knn_setup", (0, 0))[1] <= 1, names
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(es.CONFIGS))
def test_own_draw_equals_given_ids(name, make_engine):
    """The premise of the replay model: an engine that draws its own ids at iteration t gives the bits of a fresh engine
    handed the ids tests/sampler_reference.py states for (seed, t)."""
    cfg = es.CONFIGS[name]
    t = 3
    start, P = es.cloud_of(cfg, 1), es.cloud_of(cfg, 2)
    eng, fresh = make_engine(cfg), make_engine(cfg)
    try:
        eng.set_positions(start)
        eng.run(t)
        eng.set_positions(P)
        eng.step()
        fresh.set_positions(P)
        fresh.step(sampler_reference.sample_ids(cfg.E, cfg.samples, es.ENGINE_SEED, t) if cfg.draws else None)
        got, want = eng.get_positions(), fresh.get_positions()
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} values differ"
        # and a run: iterations t + 1, t + 2 on the engine that counts, the reference's ids on a fresh one
        eng.set_positions(P)
        eng.run(2)
        fresh.set_positions(P)
        fresh.run(2, sampler_reference.stream(cfg.E, cfg.samples, es.ENGINE_SEED, t + 1, 2) if cfg.draws else None)
        assert np.array_equal(eng.get_positions(), fresh.get_positions()), name
    finally:
        eng.close()
        fresh.close()


def _run_sequence(cfg, ops, make_engine, label, torch_seed=0):
    planned = es.plan(cfg, ops, make_engine, torch_seed)
    assert all(np.isfinite(want).all() for _, want in planned if isinstance(want, np.ndarray) and want.dtype == np.float32), label
    eng = make_engine(cfg)
    try:
        es.check(eng, cfg, ops, planned, torch_seed, label)
    finally:
        eng.close()


HAND_CASES = [(c, name) for c, cfg in es.CONFIGS.items() for name, ops in es.HAND_WRITTEN.items() if es.admits_all(cfg, ops)]


@pytest.mark.parametrize("config,name", HAND_CASES, ids=[f"{c}-{n}" for c, n in HAND_CASES])
def test_hand_written_sequences(config, name, make_engine):
    _run_sequence(es.CONFIGS[config], es.HAND_WRITTEN[name], make_engine, f"{config}, hand-written {name}", torch_seed=77)


@pytest.mark.parametrize("seed", es.SEEDS)
@pytest.mark.parametrize("config", list(es.CONFIGS))
def test_random_sequences(config, seed, make_engine):
    _run_sequence(es.CONFIGS[config], es.sequence(config, seed), make_engine, f"{config}, seed {seed}", torch_seed=seed)


@pytest.mark.parametrize("seed", [0, 3])
def test_two_engines_interleaved(seed, make_engine):
    """Two handles of different configurations on one device, their sequences interleaved operation by operation: each
    gives what it gives alone.  Nothing is shared between handles through a static or a thread-local; a refused call on
    one handle leaves the other's error string, and the create error, alone."""
    from graphem_rapids_amd import _native
    lib = _native.load()
    cfgs = [es.CONFIGS["fused_coarse"], es.CONFIGS["fused_wide"]]
    seqs = [es.sequence(c, seed) for c in cfgs]
    seqs[0] = seqs[0][:-1] + [es.op("refused", what="step_bad_id"), es.op("step_own"), es.op("read")]
    plans = [es.plan(c, ops, make_engine, seed + i) for i, (c, ops) in enumerate(zip(cfgs, seqs))]
    states = [es.torch_state(seed + i) for i in range(2)]
    create_error = lib.gh_last_error(None)
    engines = [make_engine(c) for c in cfgs]
    try:
        for step in range(max(map(len, seqs))):
            for i, (cfg, ops, planned) in enumerate(zip(cfgs, seqs, plans)):
                if step >= len(ops):
                    continue
                r, want = planned[step]
                others_error = lib.gh_last_error(engines[1 - i].handle)
                got = es.perform(engines[i], cfg, r, states[i])
                assert es.same(got, want), (f"{cfg.name} interleaved with {cfgs[1 - i].name}, seed {seed}: the result of operation "
                                            f"{step} ({es.show(ops[step])}) differs from a fresh engine's\n{es.show_ops(ops, step)}")
                assert lib.gh_last_error(engines[1 - i].handle) == others_error
                if r.kind == "refused" and r.args["what"] == "step_bad_id":
                    assert lib.gh_last_error(engines[i].handle) == b"sampled edge id out of range"
        assert lib.gh_last_error(None) == create_error
    finally:
        for eng in engines:
            eng.close()


# ---- the split-step entry points, in process --------------------------------------------------------------------------
WORLD, PART_S, PART_K, PART_D = 2, 64, 10, 3
FINISHES = ("own", "gathered", "overlap")
PART = es.CONFIGS["fused_embedded"]   # the 4200-vertex graph at D = 3: the shapes of the shards (ids_of, cloud_of)


def _shards(finish):
    from graphem_rapids_amd import _native
    from graphem_rapids_amd.distributed import HipShardEngine, partition_rows
    shards = []
    for r in range(WORLD):
        chunk, lo, hi = partition_rows(PART.n, WORLD, r)
        sh = HipShardEngine(PART.n, PART_D, _edges(PART.n), *es.PARAMS, PART_K, PART_S, es.ENGINE_SEED,
                            (lo, hi, 0, 0, _native.EDGES_HASHED), 0)
        if finish == "own":
            sh.rank_layout(WORLD, r, chunk, packed=True)
        elif finish == "gathered":
            sh.gather_layout(WORLD, r, chunk)
        else:
            sh.overlap_layout(WORLD, r, chunk)
        shards.append(sh)
    return shards


def _close(shards):
    for sh in shards:
        sh.eng.close()


def partitioned_sequence(seed):
    """8 operations: step_in_process with given ids, with the ranks' own draw, and set_positions on every shard."""
    rng = np.random.default_rng([9, seed])
    ops = [es.op("set_positions", cloud=2000 + seed)]
    kinds = ["step_given", "step_own", "step_own", "set_positions"]
    while len(ops) < 8:
        kind = str(rng.choice(kinds))
        s = int(rng.integers(0, 1 << 20))
        ops.append(es.op(kind, ids=s) if kind == "step_given" else es.op(kind, cloud=s) if kind == "set_positions" else es.op(kind))
    return ops


PART_HAND = {
    # under the gathered finishes: own_ids and the set-up made ahead for a draw that a given step then does not take
    "given_own_own_given_own": [es.op("set_positions", cloud=1), es.op("step_given", ids=2), es.op("step_own"), es.op("step_own"),
                                es.op("step_given", ids=3), es.op("step_own")],
    # under overlap: both parities of the patch counters, and positions set between them
    "seven_own_steps": [es.op("set_positions", cloud=4)] + [es.op("step_own")] * 3 + [es.op("set_positions", cloud=5)] + [es.op("step_own")] * 4,
}


def _partitioned(finish, ops, label):
    """The model's pass on fresh shards per step, then the operations on one set of shards with nothing in between."""
    import torch
    from graphem_rapids_amd.distributed import step_in_process
    pos, it, planned = None, 0, []
    for o in ops:
        if o.kind == "set_positions":
            pos = es.cloud_of(PART, o.args["cloud"])
            planned.append((o, pos, None))
            continue
        ids = es.ids_of(PART, o.args["ids"]) if o.kind == "step_given" else None
        model_ids = ids if ids is not None else sampler_reference.sample_ids(PART.E, PART_S, es.ENGINE_SEED, it)
        fresh = _shards(finish)
        try:
            for sh in fresh:
                sh.set_positions(pos)
            step_in_process(fresh, finish, model_ids)
            torch.cuda.synchronize()
            outs = [sh.get_positions() for sh in fresh]
        finally:
            _close(fresh)
        assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1]), f"{label}: the replay's ranks differ at {es.show(o)}"
        pos, it = outs[0], it + 1
        planned.append((o, ids, pos))
    shards = _shards(finish)
    try:
        for o, arg, _ in planned:
            if o.kind == "set_positions":
                for sh in shards:
                    sh.set_positions(arg)
            else:
                step_in_process(shards, finish, arg)
        torch.cuda.synchronize()
        outs = [sh.get_positions() for sh in shards]
    finally:
        _close(shards)
    listing = es.show_ops(ops)
    ranks_agree, as_replayed = np.array_equal(outs[0], outs[1]), np.array_equal(outs[0], pos)
    assert ranks_agree, f"{label}: the ranks differ after\n{listing}"
    assert as_replayed, f"{label}: {int((outs[0] != pos).sum())} values differ from the replay after\n{listing}"
    return planned


def _first_divergence(finish, ops, label):
    """After a failure: the same sequence cut after each step in turn, to name the first step whose result differs."""
    for upto in range(2, len(ops)):
        if ops[upto - 1].kind != "set_positions":
            _partitioned(finish, ops[:upto], f"{label}, first {upto} operations")


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("finish", FINISHES)
def test_partitioned_random_sequences(finish, seed):
    ops, label = partitioned_sequence(seed), f"finish {finish}, seed {seed}"
    try:
        _partitioned(finish, ops, label)
    except AssertionError:
        _first_divergence(finish, ops, label)
        raise


@pytest.mark.parametrize("name", list(PART_HAND))
@pytest.mark.parametrize("finish", FINISHES)
def test_partitioned_hand_written_sequences(finish, name):
    ops, label = PART_HAND[name], f"finish {finish}, hand-written {name}"
    try:
        _partitioned(finish, ops, label)
    except AssertionError:
        _first_divergence(finish, ops, label)
        raise
