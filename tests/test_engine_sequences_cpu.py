"""The generator of tests/engine_sequences.py produces what test_hip_engine_sequences.py relies on: over the seeds the GPU
test runs, every operation kind in every configuration that admits it and every (state-leaving, state-consuming) pair of
the table; the hand-written list holds the transitions named in csrc/engine.h.  Whoever changes the generator so that a
pair silently disappears gets a failure here, not a GPU test that stopped covering it.

The replay model and the comparison are run here too, against a stand-in engine in numpy that is a pure function of
(positions, iteration, arguments) -- and against one that keeps a set-up done ahead when it must not, which they must
catch."""
import numpy as np
import pytest

import engine_sequences as es
import sampler_reference


def _all_random():
    return {(name, seed): es.sequence(name, seed) for name in es.CONFIGS for seed in es.SEEDS}


def _adjacent(ops):
    return {(a.kind, b.kind) for a, b in zip(ops, ops[1:])}


def test_sequences_are_deterministic_and_well_formed():
    for (name, seed), ops in _all_random().items():
        cfg = es.CONFIGS[name]
        assert ops == es.sequence(name, seed) == es.sequence(cfg, seed)
        assert es.MIN_OPS <= len(ops) <= es.MAX_OPS, (name, seed, len(ops))
        assert ops[0].kind == "set_positions" and "cloud" in ops[0].args and ops[-1].kind == "read"
        assert es.admits_all(cfg, ops), (name, seed)
        for i, o in enumerate(ops[:-1]):
            if o.kind == "read":   # a read sits behind a mutating operation only
                assert ops[i - 1].kind in es.MUTATING, (name, seed, i)
            if o.kind in ("run_given", "run_own", "run_torch"):
                assert 1 <= o.args["t"] <= 4
        mutating = sum(o.kind in es.MUTATING for o in ops)
        reads = sum(o.kind == "read" for o in ops[:-1])
        assert reads <= mutating // 3, (name, seed)   # the other mutating operations run back to back
    assert len({tuple(map(es.show, ops)) for ops in _all_random().values()}) == len(es.CONFIGS) * len(es.SEEDS)


@pytest.mark.parametrize("name", list(es.CONFIGS))
def test_every_admitted_kind_occurs_in_every_configuration(name):
    cfg = es.CONFIGS[name]
    seen = {o.kind for seed in es.SEEDS for o in es.sequence(name, seed)}
    assert seen == {k for k in es.KINDS if es.admits(cfg, k)}
    refused = {o.args["what"] for seed in es.SEEDS for o in es.sequence(name, seed) if o.kind == "refused"}
    assert refused <= set(es.refusals(cfg))


def test_refusals_over_the_configurations():
    assert set(es.refusals(es.CONFIGS["fused_embedded"])) == set(es.REFUSALS)
    assert set(es.refusals(es.CONFIGS["all_edges"])) == {"run_negative", "inter_bad_table"}   # arange: the caller's ids are not read
    assert set(es.refusals(es.CONFIGS["no_queries"])) == {"run_negative", "step_bad_id", "run_bad_id"}
    seen = {o.args["what"] for ops in _all_random().values() for o in ops if o.kind == "refused"}
    seen |= {o.args["what"] for ops in es.HAND_WRITTEN.values() for o in ops if o.kind == "refused"}
    assert seen == set(es.REFUSALS)


def _missing_pairs(sequences):
    seen = set().union(*(_adjacent(ops) for ops in sequences))
    return [(a, b) for a, b, _ in es.PAIRS if (a, b) not in seen]


def test_every_pair_of_the_table_occurs():
    assert len(es.PAIRS) == len({(a, b) for a, b, _ in es.PAIRS}) == 43
    for a, b, state in es.PAIRS:
        assert a in es.KINDS and b in es.KINDS and state
    assert _missing_pairs(_all_random().values()) == []
    # where a plan change is half of a pair it is a flip, and the second of two given runs is the longer one
    for ops in _all_random().values():
        for a, b in zip(ops, ops[1:]):
            if (a.kind, b.kind) == ("run_given", "run_given") and (a.args["t"], b.args["t"]) == (2, 4):
                break
        else:
            continue
        break
    else:
        raise AssertionError("no run_given(2), run_given(4): d_stream_ids is never re-grown")


def test_the_pairs_come_from_the_table(monkeypatch):
    """With all but one row of the table taken away the drawn rest no longer covers it: the table is what carries the pairs,
    and taking a row away is noticed."""
    monkeypatch.setattr(es, "PAIRS", es.PAIRS[:1])
    thin = [es.sequence(name, seed) for name in es.CONFIGS for seed in es.SEEDS]
    monkeypatch.undo()
    assert len(_missing_pairs(thin)) >= 5


# the transitions the hand-written list must hold (kinds in order, anywhere in one sequence, adjacent)
TRANSITIONS = (
    ("run_own", "knn", "step_own"),
    ("run_own", "filter", "step_given"),
    ("run_own", "coarse", "run_own"),
    ("knn", "integrate", "step_given"),
    ("knn", "knn", "step_own"),
    ("split_abandoned", "step_given"),
    ("run_given", "set_positions", "run_given"),
    ("run_torch", "run_given", "run_torch"),
    ("step_own", "refused", "step_own"),
    ("timing", "run_own", "timing", "step_given", "timing", "step_own"),
    ("inter", "step_given"),
    ("run_own",) * 5 + ("set_positions", "run_own"),
    # found missing when the look-ahead was kept on purpose (DESIGN.md "Call sequences")
    ("run_own", "inter", "step_own"),
    ("run_own", "filter", "step_own"),
    ("filter", "run_own", "filter", "step_own"),
)


def test_hand_written_sequences():
    kinds = {name: tuple(o.kind for o in ops) for name, ops in es.HAND_WRITTEN.items()}

    def holds(seq, part):
        return any(seq[i:i + len(part)] == part for i in range(len(seq) - len(part) + 1))

    for part in TRANSITIONS:
        assert any(holds(seq, part) for seq in kinds.values()), part
    for name, ops in es.HAND_WRITTEN.items():
        assert ops[0].kind == "set_positions" and ops[-1].kind == "read" and len(ops) <= es.MAX_OPS, name
        assert not any(o.kind == "read" for o in ops[:-1]), name   # nothing synchronises on the way
        assert sum(es.admits_all(cfg, ops) for cfg in es.CONFIGS.values()) >= 4, name
    regrown = es.HAND_WRITTEN["stream_regrown"]
    assert regrown[1].args["t"] < regrown[3].args["t"]
    reads = [o.args["t"] for o in es.HAND_WRITTEN["torch_given_torch"] if o.kind != "set_positions" and "t" in o.args]
    assert reads == [3, 2, 3]
    assert sum(es.admits_all(cfg, ops) for cfg in es.CONFIGS.values() for ops in es.HAND_WRITTEN.values()) == 229


def test_configurations():
    assert list(es.CONFIGS) == ["block", "fused_embedded", "fused_cells", "fused_coarse", "fused_d2", "fused_wide", "fused_s300",
                                "all_edges", "grid", "ivf", "cdist", "no_queries"] == list(es.REPORTS)
    c = es.CONFIGS
    assert (c["block"].n, c["block"].E) == (2000, 8000) and all(x.E == 16800 for x in c.values() if x.name != "block")
    assert c["all_edges"].samples == 16800 and not c["all_edges"].draws and c["fused_s300"].samples == 300
    assert [x.name for x in c.values() if x.filter_ops] == ["fused_embedded", "fused_cells", "fused_coarse", "fused_d2"]
    assert es.ids_of(c["all_edges"], 3).tolist() == list(range(16800))
    ids = es.ids_of(c["block"], 3)
    assert len(ids) == len(set(ids.tolist())) == 64 and ids.max() < 8000 and np.array_equal(ids, es.ids_of(c["block"], 3))


# ---- the model and the comparison against a stand-in engine --------------------------------------------------------------
class StandIn:
    """An engine in numpy whose every result is a function of (positions, iteration, arguments).  stale: it keeps the
    set-up it made ahead for its own draw when knn_midpoints overwrites the ids (the mistake caller_ids guards against)."""

    def __init__(self, cfg, stale=False):
        self.cfg, self.stale = cfg, stale
        self.n, self.D, self.E, self.S, self.k = cfg.n, cfg.D, cfg.E, cfg.samples, cfg.k
        self.pos = np.zeros((cfg.n, cfg.D), dtype=np.float32)
        self.iter = 0
        self.sampled = None     # the ids "in d_sampled"
        self.ahead = False      # a set-up was done ahead for the own draw of iteration self.iter

    def _check(self, ids):
        if self.cfg.draws and ids is not None and ((ids < 0) | (ids >= self.E)).any():
            raise ValueError("sampled edge id out of range")

    def _own(self):
        if not self.cfg.draws:
            return np.arange(self.E, dtype=np.int32)
        if self.ahead and self.stale:
            return self.sampled
        return sampler_reference.sample_ids(self.E, self.S, es.ENGINE_SEED, self.iter)

    def _one(self, ids, own):
        w = np.float32(1 + (int(ids.astype(np.int64).sum()) % 97) / 97)
        new = self.pos + w * np.roll(self.pos, 1, axis=0) + np.float32(0.01)
        self.pos = ((new - new.mean(axis=0)) / (new.std(axis=0) + np.float32(1))).astype(np.float32)
        self.iter += 1
        self.ahead = own
        if own and self.cfg.draws:
            self.sampled = sampler_reference.sample_ids(self.E, self.S, es.ENGINE_SEED, self.iter)

    def set_positions(self, pos):
        self.pos, self.ahead = np.array(pos, dtype=np.float32), False

    def get_positions(self):
        return self.pos.copy()

    def step(self, ids=None):
        self._check(ids)
        self._one(self._own() if ids is None or not self.cfg.draws else ids, ids is None)

    def run(self, iters, stream=None):
        if iters < 0:
            raise ValueError("negative iteration count")
        if stream is not None:
            self._check(np.asarray(stream))
        for t in range(iters):
            self._one(self._own() if stream is None or not self.cfg.draws else stream[t], stream is None)

    def run_torch_sampled(self, iters, state):
        if not self.cfg.draws:
            return self.run(iters)
        from graphem_rapids_amd import _native
        return self.run(iters, _native.torch_randperm_prefix(state, self.E, self.S, iters))

    def knn_midpoints(self, ids):
        self._check(ids)
        if self.cfg.draws:
            self.sampled = ids      # the ids of the set-up done ahead are gone ...
            if not self.stale:
                self.ahead = False  # ... and so is the set-up
        return (ids[:, None].astype(np.int64) * 31 + np.arange(self.k) + int(abs(self.pos).sum() * 8)).astype(np.int32) % self.E

    step_begin = lambda self, ids=None: self._check(ids)

    def spring_forces(self):
        return self.pos - np.roll(self.pos, 1, axis=0)

    def intersection_forces(self, ids, table):
        if ((table < 0) | (table >= self.E)).any():
            raise ValueError("neighbour edge id out of range")
        return self.pos * np.float32(int(table.astype(np.int64).sum() + ids.astype(np.int64).sum()) % 13)

    def integrate_normalise(self, Fs, Fi):
        return self.pos + Fs + Fi

    def radial_topk(self, k):
        return np.argsort(-(self.pos ** 2).sum(axis=1), kind="stable")[:k].astype(np.int32)

    def set_scan_filter(self, mode):
        assert self.cfg.filter_ops and mode in ("auto", "mfma", "cells")

    def set_coarse_tau(self, mode):
        assert self.cfg.filter_ops and mode in ("auto", "on", "off")

    timing_enable = timing_reset = sync = close = lambda self, *a: None


@pytest.fixture(scope="module")
def native_library():
    from graphem_rapids_amd import _native
    _native.load()   # (host code only: torch.randperm's prefixes)


@pytest.mark.parametrize("name", ["block", "fused_coarse", "all_edges", "no_queries"])
def test_model_follows_a_history_free_engine(name, native_library):
    cfg = es.CONFIGS[name]
    sequences = [es.sequence(name, seed) for seed in es.SEEDS] + [ops for ops in es.HAND_WRITTEN.values() if es.admits_all(cfg, ops)]
    for i, ops in enumerate(sequences):
        planned = es.plan(cfg, ops, StandIn, torch_seed=i)
        assert [r.kind for r, _ in planned] == [o.kind for o in ops]
        es.check(StandIn(cfg), cfg, ops, planned, torch_seed=i, label=f"{name} #{i}")
        got_by_advance = es.plan(cfg, ops, StandIn, torch_seed=i, own_by_advance=True)
        assert all(es.same(a[1], b[1]) for a, b in zip(planned, got_by_advance))


def test_model_catches_a_set_up_kept_too_long(native_library):
    cfg = es.CONFIGS["fused_embedded"]
    ops = es.HAND_WRITTEN["own_run_search_own_step"]
    planned = es.plan(cfg, ops, StandIn)
    es.check(StandIn(cfg), cfg, ops, planned)
    with pytest.raises(AssertionError) as info:
        es.check(StandIn(cfg, stale=True), cfg, ops, planned, label="fused_embedded own_run_search_own_step")
    text = str(info.value)
    assert "fused_embedded own_run_search_own_step: the result of operation 4 (read) differs" in text
    assert "3 step_own" in text and "2 knn(ids=3)" in text   # the operations up to it
    # a call that should have been refused and was not, and a refusal nobody asked for
    lenient = type("Lenient", (StandIn,), {"_check": lambda self, ids: None})
    ops = es.HAND_WRITTEN["refused_id_between_own_steps"]
    planned = es.plan(cfg, ops, StandIn)
    with pytest.raises(AssertionError, match=r"operation 2 \(refused\(what=step_bad_id\)\) differs.*got 'no error'"):
        es.check(lenient(cfg), cfg, ops, planned)
    strict = type("Strict", (StandIn,), {"sync": lambda self: (_ for _ in ()).throw(ValueError("no"))})
    ops = [es.op("set_positions", cloud=1), es.op("sync"), es.op("read")]
    with pytest.raises(AssertionError, match=r"operation 1 \(sync\) raised ValueError"):
        es.check(strict(cfg), cfg, ops, es.plan(cfg, ops, StandIn))
