"""The capped launches of the graph analyses on the shared CSR handle, of the cascade and RR-set kernels (influence.hip,
ris.hip) and of the block-model generator, and the shapes at which tests/test_hip_launch_caps.py,
tests/test_hip_cascade_caps.py and tests/test_hip_generators.py take each of them past its cap: one table.  The caps are read out of the csrc files, so the
CPU test over this table (tests/test_launch_caps_cpu.py) fails when somebody raises a cap and a shape stops passing it,
instead of a GPU test that silently covers nothing any more.  Nothing here touches the library under test."""
import functools
import pathlib
import re
import types

import numpy as np

CSRC = pathlib.Path(__file__).resolve().parent.parent / "graphem-rapids_amd" / "csrc"

# name: the file that defines it
DEFINES = {
    "GS_BLOCK": "csr_core.h", "GS_MAX_BLOCKS": "csr_core.h",
    "CM_BLOCK": "communities.hip", "CM_MAX_BLOCKS": "communities.hip", "CM_GROUP": "communities.hip", "CM_SHORT": "communities.hip",
    "CM_LDS_SLOTS": "communities.hip",
    "PR_BLOCK": "centrality.hip", "PR_MAX_BLOCKS": "centrality.hip",
    "QUAL_BLOCK": "qual_handle.h", "QUAL_HOP_MAX_BLOCKS": "quality.hip", "QUAL_HOP_STATE_BYTES": "quality.hip",
    "CENT_DEFAULT_BUDGET": "cent_handle.h",   # the default budget of the centrality handle
    "IC_BLOCK": "influence.hip", "IC_MAX_BLOCKS": "influence.hip", "IC_PULL_DIV": "influence.hip", "IC_DEFAULT_BUDGET": "influence.hip",
    "RR_MAX_WORDS": "influence.hip", "RR_MIN_WORDS_CAP": "influence.hip",
    "RR_BLOCK": "ris.hip", "RR_MAX_BLOCKS": "ris.hip", "RR_COVER_BLOCKS": "ris.hip",
    "GEN_BLOCK": "generators.hip", "GEN_MAX_BLOCKS": "generators.hip", "GEN_DEFAULT_BUDGET": "generators.hip",
}


def parse_define(text, name):
    """The integer value of `#define name <integer expression>` in a source text: digits, + - * << and parentheses, the
    ll / ull / u suffixes dropped, a trailing comment ignored."""
    found = re.findall(rf"^[ \t]*#[ \t]*define[ \t]+{name}[ \t]+(.+?)[ \t]*(?://.*|/\*.*)?$", text, flags=re.M)
    if len(found) != 1:
        raise LookupError(f"{len(found)} definitions of {name}")
    expr = re.sub(r"\b(\d+)(?:ull|ll|u|l)\b", r"\1", found[0], flags=re.I)
    if not re.fullmatch(r"[0-9()+\-*<\s]+", expr):
        raise ValueError(f"{name} is not an integer expression: {found[0]!r}")
    return int(eval(expr, {"__builtins__": {}}))   # pylint: disable=eval-used  (digits and operators only, checked above)


@functools.lru_cache(maxsize=None)
def defines(root=CSRC):
    """Every define of DEFINES as parsed from the sources under `root`."""
    return types.SimpleNamespace(**{name: parse_define((pathlib.Path(root) / file).read_text(encoding="utf-8"), name)
                                    for name, file in DEFINES.items()})


def ceil_div(a, b):
    return -(-a // b)


def groups_in_flight(state_bytes, n, n_sources):
    """The source groups of one batch of the bit-parallel search, as gh_cent_distances and gh_qual_hop_profile size it: 24 n
    bytes a group, at most the groups there are, at most 65535 (grid.y)."""
    return max(1, min(state_bytes // (24 * n), ceil_div(n_sources, 64), 65535))


def ic_sets_per_chunk(budget, n, W, n_sets):
    """The seed sets of one chunk of gh_ic_spread: ic_bytes_per_set of csrc/influence.hip -- three (n, W) word arrays, the
    round stamp, the touched byte and three lists -- into the budget, at most the sets there are and 2^31 entries."""
    return min(max(1, budget // (n * (3 * 8 * W + 4 + 1 + 3 * 4))), n_sets, (2 ** 31 - 1) // n)


def ic_pull_min(d, sets_in_chunk, n):
    """pull_min of ic_run_levels: a level pulls from this many frontier entries on, and pushes below."""
    return max(1, sets_in_chunk * n // d.IC_PULL_DIV)


def rr_words_per_chunk(d, n, n_samples, budget=None):
    """W of ic_rr_sample: what the budget holds of one set's state, at most RR_MAX_WORDS, at most half the pull threshold in
    roots (RR_MIN_WORDS_CAP for small graphs), at most the words the samples fill."""
    W = max(1, ((d.IC_DEFAULT_BUDGET if budget is None else budget) // n - 17) // 24)
    return min(W, d.RR_MAX_WORDS, max(d.RR_MIN_WORDS_CAP, n // (2 * 64 * d.IC_PULL_DIV)), ceil_div(n_samples, 64))


def sbm_segments(sizes, segment):
    """(first segment, segments) of every block pair a <= b in the order gh_gen_sbm numbers them: a pair space of N index
    pairs is cut into ceil(N / segment) segments whatever its probability."""
    out, seg0 = [], 0
    for a, sa in enumerate(sizes):
        for b in range(a, len(sizes)):
            count = ceil_div(sa * (sa - 1) // 2 if a == b else sa * sizes[b], segment)
            out.append((seg0, count))
            seg0 += count
    return out


def pair_group_width(n, m):
    """lk_group_width of csrc/links.hip: the power of two at or above the mean degree, 4 .. 64."""
    mean = ceil_div(2 * m, n) if n else 0
    G = 4
    while G < 64 and G < mean:
        G <<= 1
    return G


# ---- the shapes ------------------------------------------------------------------------------------------------------
TILED = dict(base="plc_gnp_caveman", n0=2360, m0=7952, copies=445)   # n = 1 050 200, m = 3 538 640
LEVEL = dict(n=3000, sources=30_000)                             # gh_cent_distances: level and fill kernels
SEED = dict(n=40, sources=1_048_576 + 300)                       # gh_cent_distances: seed kernel
HOP_SEED = dict(n=40, sources=524_288 + 300)                     # gh_qual_hop_profile: seed kernel
HOP_LEVEL = dict(n=3000, D=2, sources=12_000)                    # gh_qual_hop_profile: level kernel
PAGERANK = dict(step=70_001, init=600_001, mean_degree=3)
# random pairs, and on top of them three that are u = v pairs or repeats: the last trip is then a partial one
PAIRS = {"dense130": dict(n=130, width=64, pairs=20_000, extra=3), "ba300": dict(n=300, width=8, pairs=140_000, extra=3)}
RING = dict(n=140_001)
LONG_ROWS = dict(n=4650, hubs=150, hub_degree=1500, base_degree=40)

# influence.hip and ris.hip: the shapes A - E of tests/test_hip_cascade_caps.py (graphs and expectations: tests/cascade_caps.py)
# Whether a level pushes or pulls, and how long the lists are that advance, count, reset and scatter walk, depends on the
# frontier, which only the restatement knows: `peak` is the largest number of frontier entries (vertices whose frontier
# word is non-zero in any word, over the sets of the chunk) that any level has, `touched` the entries visited in the end.
# tests/test_launch_caps_cpu.py measures both with the restatements and holds these figures to them.
FWD_PULL = dict(n=2003, sets=17, set_size=3, p=0.3, T=1000, arc_scale=0.6,            # A: er2000, no hop limit
                measured={"p": dict(peak=33_916, touched=33_967), "arcs": dict(peak=33_782, touched=33_967)})
FWD_PUSH = dict(n=17_503, out_degree=3, sets=8, set_size=1060, p=0.3, T=4033, arc_scale=0.6)   # B: one hop
REV_PULL = dict(n=40_003, degree=6, p=0.4, hops=5, samples=1250, measured=dict(words=19, peak=17_733, touched=35_970))   # C: first chunk
REV_PUSH = dict(n=262_147, in_degree=3, samples=8192, distinct_roots=8000, p=0.5, arc_scale=1.0)   # D: one hop
COVER = dict(n=300_001, sets=9003, sizes=(0, 1, 2, 63, 64, 65, 200), heavy=290_000, heavy_sets=3001, tie_low=1234,   # E
             tie_high=280_000, tie_sets=40, members=514_140)
# generators.hip: two blocks joined by p = 1e-6 and empty inside; `segment` is GH_GEN_SBM_SEGMENT of include/graphem_hip.h
SBM = dict(sizes=(550_000, 550_000), p=1e-6, segment=16_384)


# Capped launches that an older test already takes past the cap; they have no row below.
COVERED_ELSEWHERE = {
    "gh_cent_paths, CENT_MAX_BLOCKS": "test_hip_centrality.py::test_sampled_paths_at_a_million_vertices",
    "label propagation, LP_MAX_BLOCKS * 4 vertices": "test_hip_classify.py::test_label_propagation_on_a_block_model_and_a_scale_free_graph (n = 20 000)",
    "corr_*": "test_hip_correlation.py::test_accumulator_bound (n = 2 097 151)",
    "cm_best_spill_kernel, one slice": "test_hip_communities.py::test_invariance_bit_for_bit[ladder] under set_memory_budget(1)",
}
# Not covered: the per-vertex loops of a Louvain level above 1 048 576 vertices and cm_run_count / cm_run_place past a
# million runs (a Louvain restatement at that size takes minutes), and the engine.  influence.hip, ris.hip and gen_sbm_kernel
# of generators.hip are not on the shared handle but have rows below; clusters.hip is passed by
# test_hip_clusters.py::test_device_equals_host_when_workgroups_stride.


def long_row_graph(seed=0):
    """(n, (E, 2) int64 canonical edges): every row longer than CM_SHORT, and `hubs` rows longer than the LDS table of
    cm_best_long_kernel has slots.  A ring lattice of degree base_degree on the other vertices, every hub joined to
    hub_degree .. hub_degree + 63 of them at random, and all ids permuted so that the hubs lie anywhere in the row list."""
    p = LONG_ROWS
    n, H = p["n"], p["hubs"]
    R = n - H
    rng = np.random.default_rng(seed)
    v = np.arange(R, dtype=np.int64)
    parts = [np.column_stack([v, (v + k) % R]) for k in range(1, p["base_degree"] // 2 + 1)]
    for h in range(H):
        leaves = rng.choice(R, size=p["hub_degree"] + h % 64, replace=False)
        parts.append(np.column_stack([np.full(len(leaves), R + h, dtype=np.int64), leaves]))
    e = rng.permutation(n)[np.concatenate(parts)]
    e = np.sort(e, axis=1)
    return n, e[np.lexsort((e[:, 1], e[:, 0]))]


def rows(d=None):
    """The table: one dict per launch (or family of launches that share a loop) with the kernels, the define that caps it,
    the items one trip covers, the items of the GPU test's shape, and the test.  `items > per_trip` is what
    tests/test_launch_caps_cpu.py asserts for every row; a row with a `block` also holds that the last trip is a partial one
    (more than a block past the cap, and not a whole number of blocks)."""
    d = d or defines()
    gs_trip = d.GS_MAX_BLOCKS * d.GS_BLOCK
    cm_trip = d.CM_MAX_BLOCKS * d.CM_BLOCK
    n, m = TILED["n0"] * TILED["copies"], TILED["m0"] * TILED["copies"]
    G_level = groups_in_flight(d.CENT_DEFAULT_BUDGET, LEVEL["n"], LEVEL["sources"])
    G_hop = groups_in_flight(d.QUAL_HOP_STATE_BYTES, HOP_LEVEL["n"], HOP_LEVEL["sources"])
    out = [
        dict(launch="graphstats.hip, cores.hip: vertex loops", cap="GS_MAX_BLOCKS", per_trip=gs_trip, items=n, block=d.GS_BLOCK,
             kernels="gs_label_init gs_hook gs_jump cr_degree cr_select(vertex) cr_vertex_push cr_upper_count",
             test="test_tiled_*"),
        dict(launch="cores.hip: edge loops", cap="GS_MAX_BLOCKS", per_trip=gs_trip, items=m, block=d.GS_BLOCK,
             kernels="cr_select(edge) cr_support cr_edge_push", test="test_tiled_truss"),
        dict(launch="graphstats.hip, cores.hip: arc loops", cap="GS_MAX_BLOCKS", per_trip=gs_trip, items=2 * m, block=d.GS_BLOCK,
             kernels="gs_triangle cr_edge_id", test="test_tiled_triangles, test_tiled_truss"),
        dict(launch="gs_level_kernel, workgroups per group", cap="GS_MAX_BLOCKS / G", per_trip=max(1, d.GS_MAX_BLOCKS // G_level),
             items=ceil_div(LEVEL["n"], d.GS_BLOCK), G=G_level, kernels="gs_level", test="test_distances_many_groups"),
        dict(launch="gs_frontier_fill_kernel", cap="GS_MAX_BLOCKS", per_trip=gs_trip, items=G_level * LEVEL["n"], block=d.GS_BLOCK,
             last_group_from=(G_level - 1) * LEVEL["n"], kernels="gs_frontier_fill", test="test_distances_many_groups"),
        dict(launch="gs_frontier_seed_kernel (gh_cent_distances)", cap="GS_MAX_BLOCKS", per_trip=gs_trip, items=SEED["sources"],
             block=d.GS_BLOCK, one_batch=groups_in_flight(d.CENT_DEFAULT_BUDGET, SEED["n"], SEED["sources"]) == ceil_div(SEED["sources"], 64),
             kernels="gs_frontier_seed", test="test_distance_seeds_past_the_cap"),
        dict(launch="gs_frontier_seed_kernel (gh_qual_hop_profile)", cap="QUAL_HOP_MAX_BLOCKS", per_trip=d.QUAL_HOP_MAX_BLOCKS * d.GS_BLOCK,
             items=HOP_SEED["sources"], block=d.GS_BLOCK,
             one_batch=groups_in_flight(d.QUAL_HOP_STATE_BYTES, HOP_SEED["n"], HOP_SEED["sources"]) == ceil_div(HOP_SEED["sources"], 64),
             kernels="gs_frontier_seed", test="test_hop_profile_seeds_past_the_cap"),
        dict(launch="qual_hop_level_kernel, workgroups per group", cap="QUAL_HOP_MAX_BLOCKS / G",
             per_trip=max(1, d.QUAL_HOP_MAX_BLOCKS // G_hop), items=ceil_div(HOP_LEVEL["n"], d.QUAL_BLOCK), G=G_hop,
             kernels="qual_hop_level", test="test_hop_profile_many_groups"),
        dict(launch="pr_step_kernel", cap="PR_MAX_BLOCKS", per_trip=d.PR_MAX_BLOCKS * (d.PR_BLOCK // 8), items=PAGERANK["step"],
             block=d.PR_BLOCK // 8, kernels="pr_step", test="test_pagerank[70001]"),
        dict(launch="pr_check_kernel, partial sums", cap="PR_BLOCK", per_trip=d.PR_BLOCK,
             items=min(d.PR_MAX_BLOCKS, ceil_div(PAGERANK["step"], d.PR_BLOCK // 8)), kernels="pr_check", test="test_pagerank[70001]"),
        dict(launch="pr_init_kernel", cap="PR_MAX_BLOCKS", per_trip=d.PR_MAX_BLOCKS * d.PR_BLOCK, items=PAGERANK["init"], block=d.PR_BLOCK,
             kernels="pr_init", test="test_pagerank[600001]"),
        dict(launch="communities.hip: group-per-row loops", cap="CM_MAX_BLOCKS", per_trip=cm_trip // d.CM_GROUP, items=RING["n"],
             block=d.CM_BLOCK // d.CM_GROUP, kernels="cm_best_short cm_move cm_numerator cm_arc_key", test="test_louvain_ring"),
        dict(launch="cm_best_long_kernel, rows per workgroup", cap="CM_MAX_BLOCKS", per_trip=d.CM_MAX_BLOCKS, items=LONG_ROWS["n"],
             kernels="cm_best_long", test="test_louvain_long_rows"),
        dict(launch="communities.hip: vertex loops of gh_cent_modularity", cap="CM_MAX_BLOCKS", per_trip=cm_trip, items=n, block=d.CM_BLOCK,
             kernels="cm_degree cm_scatter_T", test="test_tiled_modularity_terms"),
    ]
    for name, p in PAIRS.items():
        out.append(dict(launch=f"lk_pair_kernel, {p['width']} lanes a pair ({name})", cap="GS_MAX_BLOCKS", per_trip=gs_trip // p["width"],
                        items=p["pairs"] + p["extra"], block=d.GS_BLOCK // p["width"], kernels="lk_pair", test=f"test_pair_scores[{name}]"))
    out.append(dict(launch="gen_sbm_kernel, a thread per segment", cap="GEN_MAX_BLOCKS", per_trip=d.GEN_MAX_BLOCKS * d.GEN_BLOCK,
                    items=sum(count for _, count in sbm_segments(SBM["sizes"], SBM["segment"])), block=d.GEN_BLOCK,
                    kernels="gen_sbm<false> gen_sbm<true>", test="test_hip_generators.py::test_sbm_device_equals_host_past_the_cap"))
    return out + cascade_rows(d)


def cascade_rows(d):
    """The rows of influence.hip and ris.hip.  A level kernel only works on the side of pull_min its frontier is on, so a
    row's items are 0 -- and the row fails -- when the sizing rules as the sources now state them no longer send the shape's
    frontier through the kernel the row names, or no longer give the chunk the measured figures were taken for.  Push takes
    a wave per 64 (entry, word) items and both push shapes have W a multiple of 64, so those rows have no ragged block;
    `second_trip` is what is left for the last trip, which tests/test_launch_caps_cpu.py holds to be a partial one."""
    here = "test_hip_cascade_caps.py::"
    ic_trip = d.IC_MAX_BLOCKS * d.IC_BLOCK      # (entry, word) items: a thread each, or a lane each of a wave's 64
    ic_waves = ic_trip // 64                    # ic_count_kernel: a wave per (64 touched entries, word)
    rr_trip = d.RR_MAX_BLOCKS * d.RR_BLOCK
    out = []

    a = FWD_PULL
    W = ceil_div(a["T"], 64)
    chunk = ic_sets_per_chunk(d.IC_DEFAULT_BUDGET, a["n"], W, a["sets"])
    pull_min = ic_pull_min(d, chunk, a["n"])
    peak, touched = (min(m[key] for m in a["measured"].values()) for key in ("peak", "touched"))
    whole = chunk == a["sets"]                  # the figures were measured over all the sets in one chunk
    out += [
        dict(launch="ic_pull_kernel, forward", cap="IC_MAX_BLOCKS", per_trip=ic_trip, block=d.IC_BLOCK, W=W, pull_min=pull_min,
             items=chunk * a["n"] * W if whole and peak >= pull_min else 0, kernels="ic_pull<false, false> ic_pull<false, true>",
             test=here + "test_forward_pull_past_the_cap"),
        dict(launch="ic_advance_kernel, ic_reset_kernel, forward", cap="IC_MAX_BLOCKS", per_trip=ic_trip, block=d.IC_BLOCK,
             items=peak * W if whole else 0, kernels="ic_advance ic_reset", test=here + "test_forward_pull_past_the_cap"),
        dict(launch="ic_count_kernel, forward", cap="IC_MAX_BLOCKS", per_trip=ic_waves, items=ceil_div(touched, 64) * W if whole else 0,
             kernels="ic_count", test=here + "test_forward_pull_past_the_cap"),
    ]

    b = FWD_PUSH
    W = ceil_div(b["T"], 64)
    chunk = ic_sets_per_chunk(d.IC_DEFAULT_BUDGET, b["n"], W, b["sets"])
    pull_min = ic_pull_min(d, chunk, b["n"])
    entries = b["sets"] * b["set_size"]         # round 1's frontier is the seed list
    items = entries * W if chunk == b["sets"] and entries < pull_min else 0
    out.append(dict(launch="ic_push_kernel, forward", cap="IC_MAX_BLOCKS", per_trip=ic_trip, items=items, W=W, pull_min=pull_min,
                    second_trip=items - ic_trip, kernels="ic_push<false, false> ic_push<false, true>",
                    test=here + "test_forward_push_past_the_cap"))

    c = REV_PULL
    W = rr_words_per_chunk(d, c["n"], c["samples"])
    pull_min = ic_pull_min(d, 1, c["n"])
    peak, touched = c["measured"]["peak"], c["measured"]["touched"]
    whole = W == c["measured"]["words"]         # the figures are those of the first chunk at this many words
    out += [
        dict(launch="ic_pull_kernel, reverse", cap="IC_MAX_BLOCKS", per_trip=ic_trip, block=d.IC_BLOCK, W=W, pull_min=pull_min,
             items=c["n"] * W if whole and peak >= pull_min else 0, kernels="ic_pull<true, false>",
             test=here + "test_reverse_pull_past_the_cap"),
        dict(launch="rr_scatter_kernel, ic_reset_kernel, reverse", cap="IC_MAX_BLOCKS", per_trip=ic_trip, block=d.IC_BLOCK,
             items=touched * W if whole else 0, kernels="rr_scatter ic_reset", test=here + "test_reverse_pull_past_the_cap"),
        dict(launch="ic_count_kernel, reverse", cap="IC_MAX_BLOCKS", per_trip=ic_waves, items=ceil_div(touched, 64) * W if whole else 0,
             kernels="ic_count", test=here + "test_reverse_pull_past_the_cap"),
    ]

    r = REV_PUSH
    W = rr_words_per_chunk(d, r["n"], r["samples"])
    pull_min = ic_pull_min(d, 1, r["n"])
    entries = r["distinct_roots"]               # round 1's frontier is the root list
    items = entries * W if 64 * W >= r["samples"] and entries < pull_min else 0
    out.append(dict(launch="ic_push_kernel, reverse", cap="IC_MAX_BLOCKS", per_trip=ic_trip, items=items, W=W, pull_min=pull_min,
                    second_trip=items - ic_trip, kernels="ic_push<true, false> ic_push<true, true>",
                    test=here + "test_reverse_push_past_the_cap"))

    e = COVER
    test = here + "test_coverage_kernels_past_their_caps"
    out += [
        dict(launch="rr_vscatter_kernel, rr_hit_kernel, a wave per set", cap="RR_MAX_BLOCKS", per_trip=rr_trip // 64, items=e["sets"],
             block=d.RR_BLOCK // 64, kernels="rr_vscatter rr_hit", test=test),
        dict(launch="rr_argmax_kernel", cap="RR_MAX_BLOCKS", per_trip=rr_trip, items=e["n"], block=d.RR_BLOCK, kernels="rr_argmax",
             test=test),
        dict(launch="rr_cover_kernel, a wave per set of the chosen vertex", cap="RR_COVER_BLOCKS", per_trip=d.RR_COVER_BLOCKS * d.RR_BLOCK // 64,
             items=e["heavy_sets"], block=d.RR_BLOCK // 64, kernels="rr_cover", test=test),
        dict(launch="rr_vcount_kernel", cap="RR_MAX_BLOCKS", per_trip=rr_trip, items=e["members"], block=d.RR_BLOCK, kernels="rr_vcount",
             test=test),
    ]
    return out
