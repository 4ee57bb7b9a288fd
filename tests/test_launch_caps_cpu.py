"""Every shape of tests/launch_caps.py passes the cap of its launch, the caps read out of the csrc files.  Whoever raises a
cap gets a failure here, not a GPU test that stopped covering the second trip."""
import re

import numpy as np
import pytest

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
    assert len(rows) == 16
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
    names = set(re.findall(r"^def (test_\w+)\(", (here / "test_hip_launch_caps.py").read_text(encoding="utf-8"), flags=re.M))
    for row in lc.rows():
        for name in row["test"].split(", "):
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
    """A copy of the sources with GS_MAX_BLOCKS, CM_MAX_BLOCKS and PR_MAX_BLOCKS lowered: the parsed values follow, and the
    shapes, sized against the real caps, pass the lowered ones as well; raised past the shapes, the rows fail."""
    real = lc.defines()

    def with_caps(root, factor):
        root.mkdir()
        for file in set(lc.DEFINES.values()):
            text = (lc.CSRC / file).read_text(encoding="utf-8")
            for name in ("GS_MAX_BLOCKS", "CM_MAX_BLOCKS", "PR_MAX_BLOCKS"):
                text = re.sub(rf"(#define {name} )(\d+)", lambda m: m.group(1) + str(int(int(m.group(2)) * factor)), text)
            (root / file).write_text(text, encoding="utf-8")
        return lc.defines(root)

    low = with_caps(tmp_path / "low", 0.25)
    assert (low.GS_MAX_BLOCKS, low.CM_MAX_BLOCKS, low.PR_MAX_BLOCKS) == (real.GS_MAX_BLOCKS // 4, real.CM_MAX_BLOCKS // 4, real.PR_MAX_BLOCKS // 4)
    assert (low.GS_BLOCK, low.QUAL_HOP_MAX_BLOCKS, low.CENT_DEFAULT_BUDGET) == (real.GS_BLOCK, real.QUAL_HOP_MAX_BLOCKS, real.CENT_DEFAULT_BUDGET)
    check_rows(low)
    high = with_caps(tmp_path / "high", 2)
    with pytest.raises(AssertionError):
        check_rows(high)
    failing = [row["launch"] for row in lc.rows(high) if row["items"] <= row["per_trip"]]
    assert len(failing) >= 10, failing
