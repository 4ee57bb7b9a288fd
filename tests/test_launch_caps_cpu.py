"""Every shape of tests/launch_caps.py passes the cap of its launch, the caps read out of the csrc files.  Whoever raises a
cap gets a failure here, not a GPU test that stopped covering the second trip."""
import re
import types

import numpy as np
import pytest

import cascade_caps
import launch_caps as lc
import links_reference as lref
import tiled_graphs


def check_rows(d):
    """Every row of the table under the defines d."""
    rows = lc.rows(d)
    for row in rows:
        assert row["items"] > row["per_trip"], row["launch"]
        if "block" in row:   # a ragged last trip: more than a block past the cap, and not a whole number of blocks
            assert row["items"] > row["per_trip"] + row["block"] and row["items"] % row["block"] != 0, row["launch"]
        assert row.get("one_batch", True), row["launch"]   # all the sources in one batch: one seed launch takes them all
    return {row["launch"]: row for row in rows}


def test_every_shape_passes_its_cap():
    d = lc.defines()
    rows = check_rows(d)
    assert len(rows) == 29
    # the numbers the GPU tests' docstrings quote, from the defines
    level = rows["gs_level_kernel, workgroups per group"]
    assert (level["G"], level["per_trip"], level["items"]) == (469, 8, 12)
    assert lc.ceil_div(lc.LEVEL["n"], d.GS_BLOCK) > d.GS_MAX_BLOCKS / level["G"]
    fill = rows["gs_frontier_fill_kernel"]
    assert fill["items"] == 469 * 3000 and fill["last_group_from"] > fill["per_trip"]   # the last group's words: a later trip
    assert lc.LEVEL["sources"] % 64 != 0                                               # whose unused bits are preset
    hop = rows["qual_hop_level_kernel, workgroups per group"]
    assert (hop["G"], hop["per_trip"], hop["items"]) == (188, 10, 12)
    assert lc.ceil_div(lc.HOP_LEVEL["n"], d.QUAL_BLOCK) > d.QUAL_HOP_MAX_BLOCKS / hop["G"]
    assert lc.ceil_div(lc.PAGERANK["step"], rows["pr_step_kernel"]["per_trip"]) == 2
    assert lc.ceil_div(lc.PAGERANK["init"], rows["pr_step_kernel"]["per_trip"]) == 10
    assert lc.ceil_div(lc.PAGERANK["init"], rows["pr_init_kernel"]["per_trip"]) == 2
    assert rows["pr_check_kernel, partial sums"]["items"] == 2048


def test_every_row_names_a_test_that_exists():
    here = lc.CSRC.parent.parent / "tests"

    def tests_of(file):
        return set(re.findall(r"^def (test_\w+)\(", (here / file).read_text(encoding="utf-8"), flags=re.M))

    for row in lc.rows():
        for name in row["test"].split(", "):
            file, _, name = name.rpartition("::")   # a row may name its file; test_hip_launch_caps.py otherwise
            names = tests_of(file or "test_hip_launch_caps.py")
            stem = name.split("[")[0]
            assert any(n.startswith(stem[:-1]) for n in names) if stem.endswith("*") else stem in names, row["launch"]
    for where in lc.COVERED_ELSEWHERE.values():
        file, name = where.split(" ")[0].split("::")
        assert re.search(rf"^def {name.split('[')[0]}\(", (here / file).read_text(encoding="utf-8"), flags=re.M), where


def test_the_tiled_shape_is_the_base_times_the_copies():
    b = tiled_graphs.base_values(lc.TILED["base"])
    assert (b.n, len(b.edges)) == (lc.TILED["n0"], lc.TILED["m0"])
    # a base worth tiling: several cores and trusses, many rounds, several components, triangles
    assert sorted(set(b.core.tolist())) == [0, 1, 2, 3, 4, 7, 8, 9] and sorted(set(b.truss.tolist())) == list(range(2, 10))
    assert (b.rounds, b.truss_rounds, len(np.unique(b.labels)), int(b.triangles.sum()) // 3) == (90, 33, 28, 5467)


@pytest.mark.parametrize("name", sorted(lc.PAIRS))
def test_pair_group_widths(name):
    _, n, e = lref.graph(name)
    assert n == lc.PAIRS[name]["n"] and lc.pair_group_width(n, len(lref.canonical_edges(n, e))) == lc.PAIRS[name]["width"]


def test_long_row_shape():
    d = lc.defines()
    n, edges = lc.long_row_graph()
    deg = np.bincount(edges.ravel(), minlength=n)
    assert n == lc.LONG_ROWS["n"] and len(np.unique(edges, axis=0)) == len(edges) and (edges[:, 0] < edges[:, 1]).all()
    assert int((deg > d.CM_SHORT).sum()) == n > d.CM_MAX_BLOCKS            # every row is long: a workgroup takes a second row
    hubs = np.flatnonzero(deg > d.CM_LDS_SLOTS)                            # more communities than slots in round 1: overflow
    assert len(hubs) == lc.LONG_ROWS["hubs"] and int(deg[hubs].min()) >= lc.LONG_ROWS["hub_degree"]
    assert int(np.delete(deg, hubs).max()) < d.CM_LDS_SLOTS // 4
    # by vertex id the hubs lie on both trips of the row list
    assert (hubs < n - d.CM_MAX_BLOCKS).any() and (hubs >= d.CM_MAX_BLOCKS).any()


def test_parse_define():
    text = "#define A 4096\n#define B (1ll << 30)   // bytes\n  #define C (A / 2)\n#define D 2048            /* x */\n#define E 12u\n"
    assert [lc.parse_define(text, k) for k in "ABDE"] == [4096, 1 << 30, 2048, 12]
    with pytest.raises(ValueError):
        lc.parse_define(text, "C")
    with pytest.raises(LookupError):
        lc.parse_define(text, "F")
    with pytest.raises(LookupError):
        lc.parse_define(text + "#define A 1\n", "A")


def test_the_table_follows_the_sources(tmp_path):
    """A copy of the sources with GS_MAX_BLOCKS, CM_MAX_BLOCKS, PR_MAX_BLOCKS, IC_MAX_BLOCKS and RR_MAX_BLOCKS lowered: the
    parsed values follow, and the shapes, sized against the real caps, pass the lowered ones as well; raised past the
    shapes, the rows fail."""
    real = lc.defines()

    def with_caps(root, factor):
        root.mkdir()
        for file in set(lc.DEFINES.values()):
            text = (lc.CSRC / file).read_text(encoding="utf-8")
            for name in ("GS_MAX_BLOCKS", "CM_MAX_BLOCKS", "PR_MAX_BLOCKS", "IC_MAX_BLOCKS", "RR_MAX_BLOCKS"):
                text = re.sub(rf"(#define {name} )(\d+)", lambda m: m.group(1) + str(int(int(m.group(2)) * factor)), text)
            (root / file).write_text(text, encoding="utf-8")
        return lc.defines(root)

    low = with_caps(tmp_path / "low", 0.25)
    assert (low.GS_MAX_BLOCKS, low.CM_MAX_BLOCKS, low.PR_MAX_BLOCKS) == (real.GS_MAX_BLOCKS // 4, real.CM_MAX_BLOCKS // 4, real.PR_MAX_BLOCKS // 4)
    assert (low.IC_MAX_BLOCKS, low.RR_MAX_BLOCKS) == (real.IC_MAX_BLOCKS // 4, real.RR_MAX_BLOCKS // 4)
    assert (low.GS_BLOCK, low.QUAL_HOP_MAX_BLOCKS, low.CENT_DEFAULT_BUDGET) == (real.GS_BLOCK, real.QUAL_HOP_MAX_BLOCKS, real.CENT_DEFAULT_BUDGET)
    assert (low.IC_BLOCK, low.IC_PULL_DIV, low.RR_MAX_WORDS, low.RR_COVER_BLOCKS) == (real.IC_BLOCK, real.IC_PULL_DIV, real.RR_MAX_WORDS, real.RR_COVER_BLOCKS)
    check_rows(low)
    high = with_caps(tmp_path / "high", 2)
    with pytest.raises(AssertionError):
        check_rows(high)
    failing = [row["launch"] for row in lc.rows(high) if row["items"] <= row["per_trip"]]
    assert len(failing) >= 10, failing
    assert {"ic_pull_kernel, forward", "ic_push_kernel, forward", "ic_pull_kernel, reverse", "rr_argmax_kernel"} <= set(failing)


# ---- influence.hip and ris.hip: the shapes A - E ---------------------------------------------------------------------------
def _with(d, **changed):
    return types.SimpleNamespace(**{**vars(d), **changed})


def _cascade(d):
    return {row["launch"]: row for row in lc.cascade_rows(d)}


def test_cascade_sizing_restatements():
    """The sizing rules against the figures the shapes were chosen by."""
    d = lc.defines()
    a, b, c, r = lc.FWD_PULL, lc.FWD_PUSH, lc.REV_PULL, lc.REV_PUSH
    rows = _cascade(d)
    # A: 17 sets of 16 words in one chunk, a 40-bit last word; the last set straddles the end of the first trip
    assert lc.ic_sets_per_chunk(d.IC_DEFAULT_BUDGET, a["n"], 16, a["sets"]) == 17 and a["T"] - 64 * 15 == 40
    pull = rows["ic_pull_kernel, forward"]
    assert (pull["W"], pull["pull_min"], pull["items"]) == (16, 2128, 544_816)
    assert 16 * a["n"] * 16 < pull["per_trip"] < pull["items"]
    # B: 27.2 MB a set, all 8 in one chunk; 8480 seeds stay under pull_min; the second trip holds the last set's only
    assert a["n"] * (3 * 8 * 16 + 17) == 803_203 and b["n"] * (3 * 8 * 64 + 17) == 27_182_159
    push = rows["ic_push_kernel, forward"]
    assert (push["W"], push["pull_min"], push["items"]) == (64, 8751, 542_720) and b["T"] - 64 * 63 == 1
    assert 0 < push["second_trip"] < push["per_trip"] and push["per_trip"] // 64 >= (b["sets"] - 1) * b["set_size"]
    # C: 1216 samples at 19 words, then 34 at one
    assert lc.rr_words_per_chunk(d, c["n"], c["samples"]) == 19 and c["samples"] - 64 * 19 == 34
    pull = rows["ic_pull_kernel, reverse"]
    assert (pull["pull_min"], pull["items"]) == (2500, 760_057)
    # D: the smallest n with the word cap at 128 (and three isolated vertices); the chunk state fits the default budget
    assert (r["n"] - 3) // (2 * 64 * d.IC_PULL_DIV) == d.RR_MAX_WORDS > (r["n"] - 4) // (2 * 64 * d.IC_PULL_DIV)
    assert r["n"] * (3 * 8 * 128 + 17) == 809_772_083 <= d.IC_DEFAULT_BUDGET
    push = rows["ic_push_kernel, reverse"]
    assert (push["W"], push["pull_min"], push["items"]) == (128, 16_384, 1_024_000) and 64 * push["W"] == r["samples"]
    assert 0 < push["second_trip"] < push["per_trip"]
    # E: three trips of rr_cover_kernel for the heavy vertex, two of every other kernel
    assert lc.ceil_div(lc.COVER["heavy_sets"], rows["rr_cover_kernel, a wave per set of the chosen vertex"]["per_trip"]) == 3
    assert lc.COVER["tie_low"] < rows["rr_argmax_kernel"]["per_trip"] < lc.COVER["tie_high"] < lc.COVER["heavy"]


def test_cascade_rows_fail_when_a_rule_moves():
    """Each of the constants that decide which kernel a shape's level goes through, moved so that it no longer does."""
    d = lc.defines()
    assert all(row["items"] > row["per_trip"] for row in lc.cascade_rows(d))

    def failing(**changed):
        return {row["launch"] for row in lc.cascade_rows(_with(d, **changed)) if row["items"] <= row["per_trip"]}

    assert failing(IC_PULL_DIV=32) >= {"ic_push_kernel, forward", "ic_push_kernel, reverse"}   # 8480 and 8000 entries now pull
    assert "ic_pull_kernel, forward" in failing(IC_PULL_DIV=1) and "ic_pull_kernel, reverse" in failing(IC_PULL_DIV=2)
    assert "ic_push_kernel, reverse" in failing(RR_MAX_WORDS=64)
    assert {"ic_pull_kernel, reverse", "rr_scatter_kernel, ic_reset_kernel, reverse"} <= failing(RR_MAX_WORDS=16, RR_MIN_WORDS_CAP=8)
    assert failing(RR_COVER_BLOCKS=1024) == {"rr_cover_kernel, a wave per set of the chosen vertex"}
    assert len(failing(IC_MAX_BLOCKS=4096)) == 8 and len(failing(RR_MAX_BLOCKS=4096)) == 3
    assert "ic_pull_kernel, forward" in failing(IC_DEFAULT_BUDGET=1 << 23)   # ten sets a chunk: not the measured one


def _levels_through(entries, W, pull_min, per_trip):
    """(pull levels, push levels past a trip) of a chunk's frontier sizes."""
    return [e for e in entries if e >= pull_min], [e for e in entries if e < pull_min and e * W > per_trip]


@pytest.mark.parametrize("kind", ["p", "arcs"])
def test_forward_pull_shape_reaches_the_second_trips(kind):
    """A, by the restatement: the middle levels pull over the dense state, the first two and the tail push; advance, count
    and reset walk lists longer than a trip."""
    d = lc.defines()
    rows = _cascade(d)
    _, entries, touched = cascade_caps.forward_pull_expected(kind == "arcs")
    assert (max(entries), touched) == (lc.FWD_PULL["measured"][kind]["peak"], lc.FWD_PULL["measured"][kind]["touched"])
    pull = rows["ic_pull_kernel, forward"]
    pulls, _ = _levels_through(entries, pull["W"], pull["pull_min"], pull["per_trip"])
    assert len(pulls) >= 5 and pull["items"] > pull["per_trip"]
    assert entries[0] == 51 and entries[1] < pull["pull_min"] and 0 < entries[-1] < pull["pull_min"]   # push before and after
    walk = rows["ic_advance_kernel, ic_reset_kernel, forward"]
    assert max(entries) * pull["W"] >= walk["items"] > walk["per_trip"] and touched * pull["W"] >= walk["items"]
    count = rows["ic_count_kernel, forward"]
    assert lc.ceil_div(touched, 64) * pull["W"] >= count["items"] > count["per_trip"]


def test_forward_push_shape_is_its_seed_list():
    """B and D need no search: round 1's frontier is the unique seeds, or the distinct roots."""
    n, pairs, sets, _ = cascade_caps.forward_push()
    b = lc.FWD_PUSH
    assert n == b["n"] and len(sets) == b["sets"] and all(len(np.unique(s)) == b["set_size"] for s in sets)
    assert (np.bincount(pairs[:, 0], minlength=n) == np.r_[np.full(n - 3, b["out_degree"]), 0, 0, 0]).all()
    assert pairs[:, 1].max() < n - 3 and sets[-1][-1] == n - 1
    n, pairs, trials, roots, _ = cascade_caps.reverse_push()
    r = lc.REV_PUSH
    assert n == r["n"] and len(roots) == len(trials) == r["samples"] and len(np.unique(roots)) == r["distinct_roots"]
    assert (np.bincount(pairs[:, 1], minlength=n) == np.r_[np.full(n - 3, r["in_degree"]), 0, 0, 0]).all()
    assert pairs[:, 0].max() < n - 3 and (roots == n - 2).any() and len(np.unique(trials)) < len(trials)


def test_reverse_pull_shape_reaches_the_second_trips():
    """C, by the restatement: the frontier of the first chunk reaches n / 16 entries, so the level pulls over n W words, and
    the touched list times W passes a trip of rr_scatter_kernel, ic_reset_kernel and ic_count_kernel."""
    d = lc.defines()
    rows = _cascade(d)
    (indptr, members, _), fronts = cascade_caps.reverse_pull_expected()
    m = lc.REV_PULL["measured"]
    entries, touched = fronts.entries(0), fronts.touched_entries(0)
    assert fronts.words_per_chunk == m["words"] and (max(entries), touched) == (m["peak"], m["touched"])
    assert (len(members), len(np.unique(members)), int(indptr[-1])) == (92_976, 36_169, 92_976)
    pull = rows["ic_pull_kernel, reverse"]
    pulls, _ = _levels_through(entries, pull["W"], pull["pull_min"], pull["per_trip"])
    assert len(entries) == lc.REV_PULL["hops"] and len(pulls) == 4 and entries[0] < pull["pull_min"]
    assert touched * pull["W"] == rows["rr_scatter_kernel, ic_reset_kernel, reverse"]["items"]
    assert lc.ceil_div(touched, 64) * pull["W"] == rows["ic_count_kernel, reverse"]["items"]
    assert fronts.touched_entries(1) < touched and max(fronts.entries(1)) < pull["pull_min"]   # the second chunk: 34 samples, push


def test_cover_system_shape():
    e = lc.COVER
    n, indptr, members = cascade_caps.cover_system()
    sizes = np.diff(indptr)
    assert (n, len(sizes), len(members)) == (e["n"], e["sets"], e["members"])
    assert (sizes == 0).any() and {63, 64, 65} <= set(sizes.tolist()) and sizes.max() in (200, 201)   # empty sets, sets on both sides of a wave
    count = np.bincount(members, minlength=n)
    assert count[e["heavy"]] == e["heavy_sets"] and count[e["tie_low"]] == count[e["tie_high"]] == e["tie_sets"]
    others = np.delete(count, [e["heavy"], e["tie_low"], e["tie_high"]])
    assert others.max() < e["tie_sets"]
    seeds, gains = cascade_caps.cover_expected(12)
    assert seeds[:3] == [e["heavy"], e["tie_low"], e["tie_high"]] and gains[:3].tolist() == [e["heavy_sets"], e["tie_sets"], e["tie_sets"]]


def test_sbm_shape_passes_the_generator_cap():
    """Two blocks of 550 000, joined by p = 1e-6 and empty inside: a pair space has its segments whatever its probability,
    so the launch has 36.9 M of them against 16.8 M a trip, and the only live block pair lies across the end of the first
    trip.  The segment counts (16 bytes each) and the edges fit the generator's default budget."""
    d = lc.defines()
    header = (lc.CSRC.parent.parent / "include" / "graphem_hip.h").read_text(encoding="utf-8")
    assert lc.parse_define(header, "GH_GEN_SBM_SEGMENT") == lc.SBM["segment"]
    segs = lc.sbm_segments(lc.SBM["sizes"], lc.SBM["segment"])
    assert segs == [(0, 9_231_551), (9_231_551, 18_463_135), (27_694_686, 9_231_551)]
    trip = d.GEN_MAX_BLOCKS * d.GEN_BLOCK
    n_seg = sum(count for _, count in segs)
    assert lc.ceil_div(n_seg, trip) == 3 and segs[1][0] < trip < segs[1][0] + segs[1][1]
    expected_edges = lc.SBM["p"] * lc.SBM["sizes"][0] * lc.SBM["sizes"][1]
    assert 16 * n_seg + 16 * 2 * expected_edges < d.GEN_DEFAULT_BUDGET
