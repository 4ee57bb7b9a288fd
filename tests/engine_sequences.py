"""Call sequences on one float32 engine handle: the operations, a seeded generator, hand-written sequences and a replay
model.  TEST INFRASTRUCTURE ONLY; importing it and generating sequences needs no GPU.

The property (test_hip_engine_sequences.py): what a call returns or leaves in the positions is a function of the engine's
configuration, the current positions, the iteration counter and the call's arguments -- of nothing else the handle has
done.  The model therefore replays every operation on a FRESH engine of the same configuration, started from the positions
the model believes the engine has, and every comparison is bit for bit.

An operation is a record (kind, args).  Arguments are seeds and small numbers, never arrays: the arrays are made from
them (ids_of, stream_of, cloud_of, ...) so that a sequence prints in one line and the engine under test and the model
get the same bits.

  kind               call                                              changes
  set_positions      set_positions(a new cloud | the positions scaled) positions
  step_given/_own    step(ids) / step()                                positions, iter
  run_given/_own     run(t, ids) / run(t), t in 1..4                   positions, iter
  run_torch          run_torch_sampled(t, state)                       positions, iter, the generator state
  knn                knn_midpoints(ids)                                nothing visible
  spring             spring_forces()                                   nothing
  inter              intersection_forces(ids, table)                   nothing
  integrate          integrate_normalise(Fs, Fi)                       nothing (the positions are restored)
  topk               radial_topk(k)                                    nothing
  filter / coarse    set_scan_filter / set_coarse_tau                  the plan
  timing             timing_enable(True | False), timing_reset()       nothing
  sync / read        sync() / get_positions()                          nothing
  refused            a call the library must refuse                    nothing: a refused call leaves no trace
  split_abandoned    step_begin(ids | None), nothing behind it         nothing visible
"""
from collections import namedtuple

import numpy as np

import sampler_reference

Op = namedtuple("Op", "kind args")


def op(kind, **args):
    return Op(kind, args)


def show(o):
    return o.kind + ("(" + ", ".join(f"{k}={v}" for k, v in o.args.items()) + ")" if o.args else "")


def show_ops(ops, upto=None):
    ops = ops if upto is None else ops[: upto + 1]
    return "\n".join(f"  {i:2d} {show(o)}" for i, o in enumerate(ops))


# ---- configurations ------------------------------------------------------------------------------------------------------
# The graphs are those of test_hip_dimension_sweep.py: random regular of degree 8 with 4200 vertices (16 800 edges, just over
# GH_SCAN_MIN_EDGES: the fused path) or 2000 vertices (the unfused path).  S = None: sample_size = E.
FUSED_N, UNFUSED_N, DEGREE = 4200, 2000, 8
PARAMS = (1.0, 0.2, 0.5)   # L_min, k_attr, k_inter
ENGINE_SEED = 11           # gh_params.seed: the device sampler's
SEPARATE = {"GRAPHEM_HIP_TAU_SEPARATE": "1"}

Config = namedtuple("Config", "name n D S k kw env coarse filter_ops expect absent")
Config.E = property(lambda c: c.n * DEGREE // 2)
Config.samples = property(lambda c: c.E if c.S is None else c.S)
Config.draws = property(lambda c: c.samples < c.E)       # the device sampler draws; else the ids are arange(E)
Config.queries = property(lambda c: c.k > 0)


def _config(name, n=FUSED_N, D=3, S=64, k=10, kw=None, env=None, coarse=None, filter_ops=False, expect=(), absent=()):
    return Config(name, n, D, S, k, kw or {}, env or {}, coarse, filter_ops, tuple(expect), tuple(absent))


# expect / absent: phase names of one timed step (a name ending in * stands for every name it begins); filter_ops: the
# configuration admits set_scan_filter("cells") (a fused engine, at most 3 components, at most GH_QC_SMAX queries)
CONFIGS = {c.name: c for c in (
    _config("block", n=UNFUSED_N, expect=("spring*", "knn_block_select", "integrate"), absent=("spring_scan", "stats_fix")),
    _config("fused_embedded", filter_ops=True, expect=("spring_scan", "knn_select_intersect", "stats_fix", "normalise"),
            absent=("knn_tau",)),
    _config("fused_cells", env=SEPARATE, coarse="off", filter_ops=True, expect=("knn_tau", "spring_scan")),
    _config("fused_coarse", env=SEPARATE, coarse="on", filter_ops=True, expect=("spring_scan",), absent=("knn_tau",)),
    _config("fused_d2", D=2, env=SEPARATE, filter_ops=True, expect=("knn_tau", "spring_scan")),
    _config("fused_wide", D=6, expect=("spring_scan", "knn_select_intersect"), absent=("knn_tau",)),
    _config("fused_s300", S=300, expect=("spring_scan", "knn_select_intersect"), absent=("knn_tau",)),
    # (left to itself an engine with this many queries takes the grid, which `grid` covers: the scan is asked for)
    _config("all_edges", S=None, kw={"knn_method": "scan"}, expect=("spring_scan", "stats_fix"), absent=("grid_*",)),
    _config("grid", kw={"knn_method": "grid"}, expect=("grid_build", "grid_tau_scan"), absent=("spring_scan",)),
    _config("ivf", kw={"knn_method": "ivf", "ivf_probes": -1}, expect=("ivf_probe", "ivf_scan"), absent=("spring_scan",)),
    _config("cdist", kw={"knn_distance": "cdist"}, expect=("spring_scan", "knn_select_cdist*", "cdist_replay*")),
    _config("no_queries", k=0, expect=("spring*",), absent=("spring_scan", "knn_*", "grid_*", "ivf_*", "intersect")),
)}
# what scan_filter() / coarse_tau() report right after creation (asserted once per configuration by the GPU test)
REPORTS = {"block": None, "fused_embedded": ("mfma", False), "fused_cells": ("cells", False), "fused_coarse": ("cells", True),
           "fused_d2": ("cells", False), "fused_wide": ("auto", False), "fused_s300": ("mfma", False), "all_edges": None,
           "grid": None, "ivf": None, "cdist": None, "no_queries": None}

REFUSALS = ("step_bad_id", "run_bad_id", "knn_bad_id", "run_negative", "inter_bad_table")


def refusals(cfg):
    """The refused calls a configuration admits.  With sample_size >= E the ids are arange(E) and the caller's are not
    looked at, so an id == E is not refused there; without neighbours there is no KNN table to get wrong."""
    out = ["run_negative"]
    if cfg.draws:
        out += ["step_bad_id", "run_bad_id"] + (["knn_bad_id"] if cfg.queries else [])
    if cfg.queries:
        out.append("inter_bad_table")
    return out


MUTATING = ("set_positions", "step_given", "step_own", "run_given", "run_own", "run_torch")
KINDS = MUTATING + ("knn", "spring", "inter", "integrate", "topk", "filter", "coarse", "timing", "sync", "read", "refused",
                    "split_abandoned")


def admits(cfg, kind):
    if kind in ("knn", "inter"):   # an engine without neighbours has no rows to return and no table to take
        return cfg.queries
    if kind in ("filter", "coarse"):
        return cfg.filter_ops
    return True


def admits_all(cfg, ops):
    return all(admits(cfg, o.kind) and (o.kind != "refused" or o.args["what"] in refusals(cfg)) for o in ops)


# ---- arguments from seeds ---------------------------------------------------------------------------------------------------
def ids_of(cfg, seed):
    """int32[S] distinct edge ids (arange(E) when the configuration samples every edge)."""
    if not cfg.draws:
        return np.arange(cfg.E, dtype=np.int32)
    return np.random.default_rng([1, seed]).permutation(cfg.E)[: cfg.samples].astype(np.int32)


def stream_of(cfg, seed, t):
    return np.stack([ids_of(cfg, 1000 * seed + 7 + i) for i in range(t)])


def cloud_of(cfg, seed):
    return np.random.default_rng([2, seed]).standard_normal((cfg.n, cfg.D)).astype(np.float32)


def forces_of(cfg, seed):
    rng = np.random.default_rng([3, seed])
    Fs = (0.1 * rng.standard_normal((cfg.n, cfg.D))).astype(np.float32)
    Fi = np.zeros((cfg.n, cfg.D), dtype=np.float32)
    rows = rng.choice(cfg.n, size=cfg.n // 10, replace=False)
    Fi[rows] = (0.05 * rng.standard_normal((len(rows), cfg.D))).astype(np.float32)
    return Fs, Fi


def table_of(cfg, seed):
    return np.random.default_rng([4, seed]).integers(0, cfg.E, size=(cfg.samples, cfg.k)).astype(np.int32)


def torch_state(seed):
    """uint8[5056]: the state of a torch CPU generator seeded with `seed` (the global generator is left alone)."""
    import torch
    return torch.Generator().manual_seed(int(seed)).get_state().numpy().copy()


# ---- state-leaving / state-consuming pairs ------------------------------------------------------------------------------
# (operation that leaves state behind, operation right behind it that consumes or must invalidate it, the state) -- from
# the "set / read / cleared" comments of csrc/engine.h.  test_engine_sequences_cpu.py holds the generator to this table.
PAIRS = (
    # the look-ahead: an own-draw run leaves the set-up of its next draw (and, coarse form, a filled table copy) behind
    ("run_own", "step_own", "look-ahead consumed by the draw it was made for"),
    ("step_own", "run_own", "look-ahead consumed by the draw it was made for"),
    ("run_own", "step_given", "look-ahead dropped by caller_ids"),
    ("run_own", "run_given", "look-ahead for d_sampled, ids in d_stream_ids (gh_knn_prepare)"),
    ("run_own", "run_torch", "look-ahead for d_sampled, ids in the device ring (gh_knn_prepare)"),
    ("run_own", "knn", "look-ahead dropped by caller_ids; d_sampled overwritten"),
    ("run_own", "inter", "look-ahead dropped by caller_ids; d_sampled overwritten"),
    ("run_own", "set_positions", "look-ahead dropped by gh_set_positions; coarse copy filled ahead and never consumed"),
    ("run_own", "filter", "look-ahead dropped by gh_replan when the threshold form changes"),
    ("run_own", "coarse", "look-ahead dropped by gh_replan when the threshold form changes"),
    ("run_own", "integrate", "look-ahead dropped by gh_launch_normalise"),
    ("run_own", "split_abandoned", "look-ahead consumed (own ids) or dropped (given ids) by a step that never finishes"),
    ("step_own", "step_given", "look-ahead dropped by caller_ids"),
    ("filter", "step_own", "the plan after a flip: the stand-alone set-up of the new threshold form"),
    ("coarse", "run_own", "coarse table copies after a flip (cmin_dirty, gh_cmin_claim)"),
    ("set_positions", "run_own", "iter, the sampler's key and the table copy's parity go on from where they were"),
    # gh_step_state: a search without a step leaves new0_ready / stats_reduced / tcount_reset_pending
    ("knn", "step_given", "new0_ready and stats_reduced left by a search without a step (gh_step_reset)"),
    ("knn", "step_own", "new0_ready left; the own draw's ids were overwritten in d_sampled"),
    ("knn", "integrate", "new0_ready left; integrate_normalise must not take the fused kernel's pos + Fs"),
    ("knn", "knn", "two searches, no step between them"),
    ("knn", "run_given", "new0_ready left; ids from d_stream_ids"),
    ("knn", "run_torch", "new0_ready left; ids from the device ring"),
    ("knn", "inter", "d_keys_cur moves from d_partial to d_merged"),
    ("integrate", "step_given", "d_stats / d_new of the per-phase entry point; look-ahead dropped by gh_launch_normalise"),
    ("integrate", "step_own", "d_stats / d_new of the per-phase entry point"),
    ("split_abandoned", "step_given", "step state of a split step nobody merged or finished"),
    ("split_abandoned", "step_own", "step state of a split step nobody merged or finished"),
    ("split_abandoned", "knn", "step state of a split step nobody merged or finished"),
    # buffers zero between iterations: d_acc, d_tflag, d_tcount
    ("inter", "step_given", "accumulators cleaned by inter_cleanup; d_keys_cur at d_merged"),
    ("inter", "step_own", "accumulators cleaned by inter_cleanup; d_sampled overwritten"),
    ("step_given", "inter", "accumulators cleaned by the normalise launch"),
    ("inter", "inter", "accumulators cleaned by inter_cleanup"),
    # counters, rings and buffers that outlive a call
    ("run_own", "run_own", "iter, both parities of the coarse table copies"),
    ("run_given", "run_given", "d_stream_ids reused or re-grown"),
    ("run_torch", "run_given", "d_stream_ids as the device ring, then as a stream; ring uploads undrained"),
    ("run_given", "run_torch", "d_stream_ids released and re-grown to the device ring"),
    ("run_torch", "run_torch", "ring.uploads and ring.ev of a call that returned undrained"),
    ("run_torch", "step_own", "iter moved on by a run that drew nothing on the device"),
    ("refused", "step_own", "a refused call leaves no trace"),
    ("step_own", "refused", "a refused call leaves the look-ahead alone"),
    ("timing", "run_own", "timer slots"),
    ("timing", "step_given", "timer slots"),
    ("run_own", "timing", "timing_reset synchronises and resolves pending events"),
)


def pair_admitted(cfg, pair):
    return admits(cfg, pair[0]) and admits(cfg, pair[1])


# ---- the generator -----------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(6))   # the seeds test_random_sequences runs per configuration
MIN_OPS, MAX_OPS = 10, 16


def _random_op(cfg, kind, rng, prev=None):
    """An operation of `kind` with arguments drawn from rng.  prev: the operation in front of it (an `inter` behind a
    `knn` takes that search's ids and rows)."""
    s = int(rng.integers(0, 1 << 20))
    t = int(rng.integers(1, 5))
    if kind == "set_positions":
        return op(kind, cloud=s) if rng.random() < 0.6 else op(kind, scale=float(rng.choice([0.5, 1.5, 3.0])))
    if kind in ("step_given", "knn"):
        return op(kind, ids=s)
    if kind == "run_given":
        return op(kind, t=t, ids=s)
    if kind in ("run_own", "run_torch"):
        return op(kind, t=t)
    if kind == "inter":
        if prev is not None and prev.kind == "knn":
            return op(kind, ids=prev.args["ids"], table="knn")
        return op(kind, ids=s, table=int(rng.integers(0, 1 << 20)))
    if kind == "integrate":
        return op(kind, forces=s)
    if kind == "topk":
        return op(kind, k=int(rng.integers(1, 65)))
    if kind == "filter":
        return op(kind, mode=str(rng.choice(["flip", "flip", "auto", "mfma", "cells"])))
    if kind == "coarse":
        return op(kind, mode=str(rng.choice(["flip", "flip", "auto", "on", "off"])))
    if kind == "timing":
        return op(kind, call=str(rng.choice(["on", "off", "reset"])))
    if kind == "refused":
        return op(kind, what=str(rng.choice(refusals(cfg))))
    if kind == "split_abandoned":
        return op(kind, ids=None) if rng.random() < 0.4 else op(kind, ids=s)
    return op(kind)   # step_own, spring, sync, read


def sequence(config, seed):
    """10 to 16 operations for the configuration (a name or a Config): set_positions first, read last, a read behind a
    random third of the mutating operations only.  Deterministic per (config, seed).

    Over SEEDS every admitted kind occurs in every configuration and every pair of PAIRS occurs somewhere: sequence number
    g = 6 * (index of the configuration) + seed carries the pairs g and g + 72 / 2 of the table (the next admitted ones)
    and every sixth admitted kind, as blocks that stay together; the rest is drawn."""
    cfg = CONFIGS[config] if isinstance(config, str) else config
    ci = list(CONFIGS).index(cfg.name)
    rng = np.random.default_rng([5, ci, seed])
    g = len(SEEDS) * ci + seed

    def admitted_pair(j):
        for d in range(len(PAIRS)):
            if pair_admitted(cfg, PAIRS[(j + d) % len(PAIRS)]):
                return PAIRS[(j + d) % len(PAIRS)]
        raise AssertionError("no pair admitted")

    blocks = []
    for j in (g, g + len(SEEDS) * len(CONFIGS) // 2):
        a, b, _ = admitted_pair(j)
        # (a plan change that belongs to a pair is a flip: "auto" or the mode in use would change nothing)
        first = op(a, mode="flip") if a in ("filter", "coarse") else _random_op(cfg, a, rng)
        second = op(b, mode="flip") if b in ("filter", "coarse") else _random_op(cfg, b, rng, prev=first)
        if (a, b) == ("run_given", "run_given"):   # the second stream is the longer one: d_stream_ids is re-grown
            first, second = op(a, t=2, ids=first.args["ids"]), op(b, t=4, ids=second.args["ids"])
        blocks.append([first, second])
    have = {o.kind for blk in blocks for o in blk} | {"set_positions", "read"}
    kinds = [k for k in KINDS if admits(cfg, k)]
    for kind in kinds[seed % len(SEEDS)::len(SEEDS)]:
        if kind not in have:
            blocks.append([_random_op(cfg, kind, rng)])
            have.add(kind)
    body_len = int(rng.integers(8, 12))
    fill = [k for k in kinds if k != "read"]
    while sum(len(b) for b in blocks) < body_len:
        blocks.append([_random_op(cfg, str(rng.choice(fill)), rng)])
    order = rng.permutation(len(blocks))
    ops = [op("set_positions", cloud=1000 + seed)]
    inside = set()   # indices whose successor belongs to the same block: no read goes between them
    for b in order:
        for i, o in enumerate(blocks[b]):
            if i + 1 < len(blocks[b]):
                inside.add(len(ops))
            ops.append(o)
    mutating = [i for i, o in enumerate(ops) if o.kind in MUTATING and i not in inside and i + 1 < len(ops)
                and ops[i + 1].kind != "read"]
    n_reads = max(0, min(len([o for o in ops if o.kind in MUTATING]) // 3, len(mutating), MAX_OPS - 1 - len(ops)))
    for i in sorted(rng.choice(mutating, size=n_reads, replace=False).tolist() if n_reads > 0 else [], reverse=True):
        ops.insert(i + 1, op("read"))
    if ops[-1].kind != "read":
        ops.append(op("read"))
    assert MIN_OPS <= len(ops) <= MAX_OPS, len(ops)
    return ops


# ---- the hand-written sequences: one per transition named in the comments of csrc/engine.h ---------------------------------
_START = op("set_positions", cloud=1)
HAND_WRITTEN = {
    "own_run_search_own_step": [_START, op("run_own", t=2), op("knn", ids=3), op("step_own"), op("read")],
    "own_run_filter_flip_given_step": [_START, op("run_own", t=2), op("filter", mode="flip"), op("step_given", ids=4), op("read")],
    "own_run_coarse_flip_own_run": [_START, op("run_own", t=2), op("coarse", mode="flip"), op("run_own", t=2), op("read")],
    "search_integrate_given_step": [_START, op("knn", ids=5), op("integrate", forces=6), op("step_given", ids=7), op("read")],
    "two_searches_own_step": [_START, op("knn", ids=8), op("knn", ids=9), op("step_own"), op("read")],
    "abandoned_split_given_step": [_START, op("split_abandoned", ids=10), op("step_given", ids=11), op("read")],
    "abandoned_own_split_own_step": [_START, op("run_own", t=1), op("split_abandoned", ids=None), op("step_own"), op("read")],
    "stream_regrown": [_START, op("run_given", t=3, ids=12), op("set_positions", cloud=13), op("run_given", t=4, ids=14),
                       op("read")],
    "torch_given_torch": [_START, op("run_torch", t=3), op("run_given", t=2, ids=15), op("run_torch", t=3), op("read")],
    "refused_between_own_steps": [_START, op("step_own"), op("refused", what="run_negative"), op("step_own"), op("read")],
    "refused_id_between_own_steps": [_START, op("step_own"), op("refused", what="step_bad_id"), op("step_own"), op("read")],
    "refused_search_between_own_steps": [_START, op("step_own"), op("refused", what="knn_bad_id"), op("step_own"), op("read")],
    "refused_stream_and_table": [_START, op("run_own", t=2), op("refused", what="run_bad_id"),
                                 op("refused", what="inter_bad_table"), op("run_own", t=1), op("read")],
    "timing_on_reset_off": [_START, op("timing", call="on"), op("run_own", t=2), op("timing", call="reset"),
                            op("step_given", ids=16), op("timing", call="off"), op("step_own"), op("read")],
    "inter_before_given_step": [_START, op("inter", ids=17, table=18), op("step_given", ids=19), op("read")],
    "searched_inter_before_own_step": [_START, op("run_own", t=1), op("knn", ids=20), op("inter", ids=20, table="knn"),
                                       op("step_own"), op("read")],
    "both_parities": [_START] + [op("run_own", t=1)] * 5 + [op("set_positions", cloud=21), op("run_own", t=1), op("read")],
    # (a search behind the own run would hide a look-ahead that caller_ids kept: gh_knn_prepare compares the ids' source and
    # drops it.  The intersection entry point has no set-up of its own, so only caller_ids stands between its ids in
    # d_sampled and the next own step, which would take the set-up made ahead and intersect with the caller's ids)
    "own_run_inter_own_step": [_START, op("run_own", t=2), op("inter", ids=23, table=24), op("step_own"), op("read")],
    # (an own step behind the flip: a given one drops the look-ahead through caller_ids whatever gh_replan did)
    "own_run_filter_flip_own_step": [_START, op("run_own", t=2), op("filter", mode="flip"), op("step_own"), op("read")],
    "filter_round_trip_own_steps": [_START, op("run_own", t=1), op("filter", mode="flip"), op("run_own", t=2),
                                    op("filter", mode="flip"), op("step_own"), op("read")],
    # (the counter of published thresholds stands at S after a given step's fused launch, which no set-up made ahead has
    # zeroed; a look-ahead made in another threshold form and kept across the flip back would leave it there)
    "given_step_filter_round_trip_own_step": [_START, op("step_given", ids=25), op("filter", mode="flip"), op("run_own", t=1),
                                              op("filter", mode="flip"), op("step_own"), op("read")],
    "given_step_launch_form_round_trip_own_step": [_START, op("step_given", ids=26), op("coarse", mode="off"),
                                                   op("filter", mode="flip"), op("run_own", t=1), op("filter", mode="flip"),
                                                   op("step_own"), op("read")],
    "own_run_integrate_own_step": [_START, op("run_own", t=2), op("integrate", forces=22), op("step_own"), op("read")],
    "torch_back_to_back_own": [_START, op("run_torch", t=4), op("run_torch", t=4), op("run_torch", t=1), op("step_own"),
                               op("read")],
}


# ---- the replay model --------------------------------------------------------------------------------------------------------
class Model:
    """What the engine under test must hold after each operation, from fresh engines.  make_engine(cfg) creates an engine
    of the configuration as it is right after creation; the model applies the filter / coarse requests made so far."""

    def __init__(self, cfg, make_engine, torch_seed=0, own_by_advance=False):
        """own_by_advance: give a fresh engine its iteration counter by run(t) + set_positions instead of handing it the
        sampler reference's ids (not needed while test_own_draw_equals_given_ids holds)."""
        self.cfg, self.make_engine = cfg, make_engine
        self.pos = None
        self.iter = 0
        self.state = torch_state(torch_seed)
        self.filter = None          # the last set_scan_filter request, None: never called
        self.coarse = None          # the last set_coarse_tau request
        self.filter_now = (REPORTS[cfg.name] or ("mfma", False))[0]   # what scan_filter() reports
        self.coarse_now = cfg.coarse or "auto"
        self.own_by_advance = own_by_advance

    def fresh(self):
        eng = self.make_engine(self.cfg)
        if self.filter is not None:
            eng.set_scan_filter(self.filter)
        if self.coarse is not None:
            eng.set_coarse_tau(self.coarse)
        eng.set_positions(self.pos)
        return eng

    def _own_ids(self, t):
        """The ids the device sampler draws in iterations iter .. iter + t - 1; None where the engine uses arange."""
        if not self.cfg.draws:
            return None
        return sampler_reference.stream(self.cfg.E, self.cfg.samples, ENGINE_SEED, self.iter, t)

    def _advance(self, t, ids, step=False, own=False):
        """Positions after t iterations from the model's, with the given (t, S) ids (None: arange); step: by step(), the
        call under test being one; own: the ids are the engine's own draw."""
        eng = self.fresh()
        try:
            if self.own_by_advance and own and ids is not None and self.iter:
                eng.run(self.iter)
                eng.set_positions(self.pos)
                ids = None
            if step:
                eng.step(None if ids is None else ids[0])
            else:
                eng.run(t, ids)
            self.pos = eng.get_positions()
        finally:
            eng.close()
        self.iter += t

    def resolve(self, o):
        """The operation with everything the engine under test needs made concrete: arrays for seeds, modes for flips."""
        cfg, a = self.cfg, dict(o.args)
        if o.kind == "set_positions":
            a["pos"] = cloud_of(cfg, a["cloud"]) if "cloud" in a else (self.pos * np.float32(a["scale"])).astype(np.float32)
        elif o.kind in ("step_given", "knn"):
            a["ids_array"] = ids_of(cfg, a["ids"])
        elif o.kind == "split_abandoned":
            a["ids_array"] = None if a["ids"] is None else ids_of(cfg, a["ids"])
        elif o.kind == "run_given":
            a["ids_array"] = stream_of(cfg, a["ids"], a["t"])
        elif o.kind == "inter":
            a["ids_array"] = ids_of(cfg, a["ids"])
            a["table_array"] = None if a["table"] == "knn" else table_of(cfg, a["table"])   # "knn": filled in by expect()
        elif o.kind == "integrate":
            a["Fs"], a["Fi"] = forces_of(cfg, a["forces"])
        elif o.kind == "filter" and a["mode"] == "flip":
            a["mode"] = "mfma" if self.filter_now == "cells" else "cells"
        elif o.kind == "coarse" and a["mode"] == "flip":
            a["mode"] = "off" if self.coarse_now == "on" else "on"
        return Op(o.kind, a)

    def expect(self, o):
        """(resolved operation, expected result) and the model moved past it.  The result is what the call returns, or for
        `read` the positions; None where there is nothing to compare."""
        cfg = self.cfg
        r = self.resolve(o)
        a, kind = r.args, r.kind
        want = None
        if kind == "set_positions":
            self.pos = a["pos"]
        elif kind == "step_given":
            self._advance(1, a["ids_array"][None, :] if cfg.draws else None, step=True)
        elif kind == "run_given":
            self._advance(a["t"], a["ids_array"] if cfg.draws else None)
        elif kind == "step_own":
            self._advance(1, self._own_ids(1), step=True, own=True)
        elif kind == "run_own":
            self._advance(a["t"], self._own_ids(a["t"]), own=True)
        elif kind == "run_torch":
            ids = None
            if cfg.draws:   # (arange otherwise: no randomness consumed, the state stays)
                from graphem_rapids_amd import _native
                ids = _native.torch_randperm_prefix(self.state, cfg.E, cfg.samples, a["t"])
            self._advance(a["t"], ids)
            want = self.state.copy()
        elif kind in ("knn", "spring", "inter", "integrate", "topk"):
            eng = self.fresh()
            try:
                if kind == "knn":
                    want = eng.knn_midpoints(a["ids_array"])
                elif kind == "spring":
                    want = eng.spring_forces()
                elif kind == "inter":
                    if a["table_array"] is None:
                        a["table_array"] = eng.knn_midpoints(a["ids_array"])
                        eng.close()
                        eng = self.fresh()
                    want = eng.intersection_forces(a["ids_array"], a["table_array"])
                elif kind == "integrate":
                    want = eng.integrate_normalise(a["Fs"], a["Fi"])
                else:
                    want = eng.radial_topk(a["k"])
            finally:
                eng.close()
        elif kind == "filter":
            self.filter = a["mode"]
            self.filter_now = a["mode"] if a["mode"] != "auto" else (REPORTS[cfg.name] or ("mfma", False))[0]
        elif kind == "coarse":
            self.coarse = self.coarse_now = a["mode"]
        elif kind == "read":
            want = self.pos.copy()
        elif kind == "refused":
            want = "ValueError"
        return r, want


def perform(eng, cfg, r, state):
    """Runs the resolved operation r on the engine under test; `state`: its torch generator state (updated in place).
    Returns what the model's expect() returns for it."""
    a, kind = r.args, r.kind
    if kind == "set_positions":
        eng.set_positions(a["pos"])
    elif kind == "step_given":
        eng.step(a["ids_array"])
    elif kind == "step_own":
        eng.step()
    elif kind == "run_given":
        eng.run(a["t"], a["ids_array"])
    elif kind == "run_own":
        eng.run(a["t"])
    elif kind == "run_torch":
        eng.run_torch_sampled(a["t"], state)
        return state.copy()
    elif kind == "knn":
        return eng.knn_midpoints(a["ids_array"])
    elif kind == "spring":
        return eng.spring_forces()
    elif kind == "inter":
        return eng.intersection_forces(a["ids_array"], a["table_array"])
    elif kind == "integrate":
        return eng.integrate_normalise(a["Fs"], a["Fi"])
    elif kind == "topk":
        return eng.radial_topk(a["k"])
    elif kind == "filter":
        eng.set_scan_filter(a["mode"])
    elif kind == "coarse":
        eng.set_coarse_tau(a["mode"])
    elif kind == "timing":
        {"on": lambda: eng.timing_enable(True), "off": lambda: eng.timing_enable(False), "reset": eng.timing_reset}[a["call"]]()
    elif kind == "sync":
        eng.sync()
    elif kind == "read":
        return eng.get_positions()
    elif kind == "split_abandoned":
        eng.step_begin(a["ids_array"])
    elif kind == "refused":
        try:
            refused_call(eng, cfg, a["what"])
        except ValueError:
            return "ValueError"
        return "no error"
    else:
        raise AssertionError(f"unknown operation {kind}")
    return None


def refused_call(eng, cfg, what):
    bad = ids_of(cfg, 0).copy()
    bad[len(bad) // 2] = cfg.E   # one past the last edge
    if what == "step_bad_id":
        eng.step(bad)
    elif what == "run_bad_id":
        eng.run(2, np.stack([ids_of(cfg, 1), bad]))   # (the first row is fine: nothing of it may be run)
    elif what == "knn_bad_id":
        eng.knn_midpoints(bad)
    elif what == "run_negative":
        eng.run(-1)
    elif what == "inter_bad_table":
        table = table_of(cfg, 0)
        table[-1, -1] = cfg.E
        eng.intersection_forces(ids_of(cfg, 0), table)
    else:
        raise AssertionError(f"unknown refused call {what}")


def same(got, want):
    if want is None:
        return got is None
    if isinstance(want, str):
        return got == want
    return isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want)


def plan(cfg, ops, make_engine, torch_seed=0, **kw):
    """[(resolved operation, expected result)] of the whole sequence: the model's pass, before the engine under test
    runs anything (so that its calls go out back to back)."""
    model = Model(cfg, make_engine, torch_seed, **kw)
    return [model.expect(o) for o in ops]


def check(eng, cfg, ops, planned, torch_seed=0, label=""):
    """Runs the planned sequence on the engine under test and asserts every result; the message names the first
    operation whose result differs and lists the operations up to it."""
    state = torch_state(torch_seed)
    for i, (r, want) in enumerate(planned):
        try:
            got = perform(eng, cfg, r, state)
        except Exception as exc:   # pylint: disable=broad-exception-caught
            raise AssertionError(f"{label}: operation {i} ({show(ops[i])}) raised {type(exc).__name__}: {exc}\n"
                                 f"{show_ops(ops, i)}") from exc
        if not same(got, want):
            detail = ""
            if isinstance(want, np.ndarray) and isinstance(got, np.ndarray) and got.shape == want.shape:
                bad = np.argwhere(got != want)
                detail = f": {len(bad)} of {want.size} values differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
            elif not isinstance(want, np.ndarray):
                detail = f": got {got!r}, want {want!r}"
            raise AssertionError(f"{label}: the result of operation {i} ({show(ops[i])}) differs from a fresh engine's{detail}\n"
                                 f"{show_ops(ops, i)}")
