"""Checks of the edge-list parser that do not care which path runs them: tests/test_datasets_cpu.py calls them with
device_id = -1 (the library's host path), tests/test_hip_datasets.py with device_id = 0.  The yardsticks are the
reference's own output (tests/golden/snap_fb_synth.npz, datasets_ref.npz), the rule restated in Python
(tests/datasets_reference.py) and, where it accepts the text, load_snap_edge_list."""
import hashlib

import numpy as np
import pytest

import datasets_reference as ref
import datasets_synth
import snap_synth
from conftest import load_golden
from graphem_rapids_amd import _native, load_snap_edge_list, parse_edge_list

BLANKS = [0x09, 0x0B, 0x0C, 0x1C, 0x1D, 0x1E, 0x1F, 0x20]

GRAMMAR = {
    "no final terminator": b"1 2\n3 4",
    "cr lf": b"1 2\r\n3 4\r\n",
    "lone cr": b"1 2\r3 4\r",
    "mixed terminators": b"1 2\n3 4\r\n5 6\r7 8\n\r9 10\r\r\n11 12",
    "blank lines": b"\n\n1 2\n\n\n3 4\n\n",
    "blank lines cr lf": b"\r\n\r\n1 2\r\n\r\n",
    "leading and trailing blanks": b"  \t1 2 \t \n\t3\t4\t\n",
    "signs and zeros": b"+7 -3\n007 0000000000000000000000012\n-0 +0\n",
    "int64 ends": b"9223372036854775807 -9223372036854775808\n-9223372036854775808 0\n",
    "garbage in column 3": b"1 2 zzz\n3 4 0.5 1e-3\n5 6 1_0 \xd9\xa3\n",
    "one-field garbage line": b"1 2\nxyz\n3 4\n#\n-\n",
    "comments first middle last": b"# a\n#1 2\n1 2\n# b c d\n3 4\n#last 5 6",
    "comment of blanks only line": b"1 2\n \t \n3 4\n",
    "empty": b"",
    "comments only": b"# x\n# y 1 2\n",
    "terminators only": b"\n\r\n\r\r\n",
    "one row": b"4 9\n",
    "one row no terminator": b"4 9",
    "repeats both directions self-loops": b"5 3\n3 5\n5 3\n4 4\n3 9\n9 9\n",
}
for _c in BLANKS:
    GRAMMAR["separator 0x%02X" % _c] = b"5" + bytes([_c]) + b"6\n" + bytes([_c]) + b"7" + bytes([_c, _c]) + b"8" + bytes([_c]) + b"\n"

# name -> (format, bytes, the 1-based line the error names, the field it quotes)
ERRORS = {
    "comment after a blank": ("snap", b"1 2\n # x y\n", 2, "#"),
    "letter in field 2": ("snap", b"1 2\n3 4\n1 2x\n", 3, "2x"),
    "underscore": ("snap", b"1_0 2\n", 1, "1_0"),
    "overflow": ("edges", b"9223372036854775808 1", 1, "9223372036854775808"),
    "negative overflow": ("edges", b"1 2\n3 -9223372036854775809", 2, "-9223372036854775809"),
    "lone sign": ("snap", b"5 6\n- 1\n", 2, "-"),
    "non-ascii digit": ("snap", "1 2\n٣ 4\n".encode("utf-8"), 2, None),
    "percent line in an mtx body": ("mtx", b"%%MM\n3 3 2\n1 2\n% a b\n2 3\n", 4, "%"),
    "mtx label int64 min": ("mtx", b"%h\n1 1 1\n-9223372036854775808 5\n", 3, "-9223372036854775808"),
    "two bad lines": ("snap", b"1 2\nx y\n3 4\nz w\n", 2, "x"),
    "cr lf counted once": ("snap", b"1 2\r\n3 4\r\n\r\n5 q\r\n6 7\r\n", 4, "q"),
    "lone cr counted": ("snap", b"1 2\r3 4\r5 q\r", 3, "q"),
}


def same(got, want):
    """(vertices, edges) equal to the last bit, int64, in the reference's shapes."""
    for g, w, shape in zip(got, want, ((-1,), (-1, 2))):
        w = np.asarray(w, dtype=np.int64).reshape(shape)
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w)


def all_modes():
    return [(d, v) for d in (False, True) for v in ("edges", "rows")]


def check_against_restatement(data, fmt, device_id, **kw):
    for directed, vfrom in all_modes():
        for relabel in (False, True):
            same(parse_edge_list(data, fmt, directed, relabel, vfrom, device_id, **kw), ref.parse(data, fmt, directed, relabel, vfrom))


def check_reference_snap(device_id):
    text, _ = snap_synth.synth_text()
    gold = load_golden("snap_fb_synth")
    assert snap_synth.text_sha1(text) == str(gold["text_sha1"])
    data = text.encode("utf-8")
    same(parse_edge_list(data, "snap", False, False, "edges", device_id), (gold["vertices"], gold["edges"]))
    vertices, edges = parse_edge_list(data, "snap", True, False, "edges", device_id)
    assert vertices.dtype == np.int64 and np.array_equal(vertices, gold["vertices_directed"])
    assert edges.dtype == np.int64 and len(edges) == int(gold["n_edges_directed"])
    assert hashlib.sha1(np.ascontiguousarray(edges).tobytes()).hexdigest() == str(gold["edges_directed_sha1"])


def check_reference_netrepo(device_id):
    gold = load_golden("datasets_ref")
    for kind, text in (("mtx", datasets_synth.mtx_text()), ("edges", datasets_synth.edges_text())):
        assert datasets_synth.text_sha1(text) == str(gold[kind + "_text_sha1"])
        for directed in (False, True):
            tag = kind + ("_directed" if directed else "_undirected")
            same(parse_edge_list(text.encode("utf-8"), kind, directed, False, "rows", device_id),
                 (gold[tag + "_vertices"], gold[tag + "_edges"]))


def check_grammar(name, device_id, tmp_path):
    data = GRAMMAR[name]
    for fmt in ("snap", "edges"):
        check_against_restatement(data, fmt, device_id)
    path = tmp_path / "case.txt"
    path.write_bytes(data)
    for directed in (False, True):
        for relabel in (False, True):
            try:
                want = load_snap_edge_list(path, directed=directed, relabel=relabel)
            except Exception:  # pylint: disable=broad-exception-caught
                continue                                 # a text that one does not take
            same(parse_edge_list(data, "snap", directed, relabel, "edges", device_id), want)


def check_error(name, device_id):
    fmt, data, line, field = ERRORS[name]
    with pytest.raises(ValueError, match=r"^line %d: " % line):
        ref.parse(data, fmt)
    for directed, vfrom in all_modes():
        with pytest.raises(ValueError, match=r"^line %d: " % line) as info:
            parse_edge_list(data, fmt, directed, True, vfrom, device_id)
        if field is not None:
            assert "'" + field + "'" in str(info.value)


def check_mtx_header(device_id):
    body = ["1 2", "2 3 0.5", "5 1"]
    want = (np.array([0, 1, 2, 4]), np.array([[0, 1], [1, 2], [4, 0]]))
    head = ["%%MatrixMarket matrix coordinate pattern general", "% a comment", "%", "%5 5 3", "5 5 3"]
    for eol in ("\n", "\r\n", "\r"):
        data = (eol.join(head + body) + eol).encode()
        same(parse_edge_list(data, "mtx", True, False, "rows", device_id), want)   # the size line is no edge
        check_against_restatement(data, "mtx", device_id)
        # a blank line right after the '%' run is the one skipped line: "5 5 3" is then a row
        data = (eol.join(head[:4] + [""] + head[4:] + body) + eol).encode()
        same(parse_edge_list(data, "mtx", True, False, "rows", device_id),
             (np.array([0, 1, 2, 4]), np.array([[4, 4], [0, 1], [1, 2], [4, 0]])))
        check_against_restatement(data, "mtx", device_id)
    for data in (b"3 3 1\n1 2\n", b"% only comments\n%\n", b"%x\n3 3 0", b"", b"%"):
        check_against_restatement(data, "mtx", device_id)
    same(parse_edge_list(b"3 3 1\n1 2\n", "mtx", True, False, "rows", device_id), (np.array([0, 1]), np.array([[0, 1]])))


def check_results(device_id):
    data = datasets_synth.edges_text().encode()
    for directed, vfrom in all_modes():
        vertices, raw = parse_edge_list(data, "edges", directed, False, vfrom, device_id)
        ranks, rel = parse_edge_list(data, "edges", directed, True, vfrom, device_id)
        assert np.array_equal(ranks, np.arange(len(vertices))) and np.array_equal(vertices[rel], raw)
    check_against_restatement(data, "edges", device_id)
    loops = b"1 1\n2 2\n1 1\n"
    same(parse_edge_list(loops, "snap", False, False, "edges", device_id), ([], []))
    same(parse_edge_list(loops, "snap", False, False, "rows", device_id), ([1, 2], []))
    same(parse_edge_list(loops, "snap", True, False, "edges", device_id), ([1, 2], [[1, 1], [2, 2], [1, 1]]))
    check_against_restatement(loops, "snap", device_id)
    rng = np.random.default_rng(5)
    few = rng.integers(0, 10, size=(50000, 2)) * 37 + 3
    check_against_restatement("".join("%d\t%d\n" % (a, b) for a, b in few).encode(), "snap", device_id)
    wide = np.array([-2 ** 63, -2 ** 62 - 1, -5, -1, 0, 1, 2 ** 31, 2 ** 32 + 1, 2 ** 62, 2 ** 63 - 1], dtype=np.int64)
    rows = wide[rng.integers(0, len(wide), size=(400, 2))]
    data = "".join("%d %d\n" % (a, b) for a, b in rows).encode()
    check_against_restatement(data, "snap", device_id)
    vertices, _ = parse_edge_list(data, "snap", True, False, "rows", device_id)
    assert np.array_equal(vertices, wide)                # signed order


def check_handles(device_id):
    first, second = datasets_synth.edges_text().encode(), GRAMMAR["mixed terminators"]
    a, b = _native.EdgeListParser(device_id), _native.EdgeListParser(device_id)
    try:
        def run(h, data, directed):
            h.parse(data, "edges", directed, "edges")
            return h.vertices(), h.edges(False)
        want_first, want_second = ref.parse(first, "edges", False), ref.parse(second, "edges", True)
        same(run(a, first, False), want_first)
        same(run(b, second, True), want_second)          # two handles at once
        same((a.vertices(), a.edges(False)), want_first)
        same(run(a, second, True), want_second)          # a second parse on one handle, other text and mode
        same(run(a, first, False), want_first)
        with pytest.raises(ValueError, match="^line 2: "):
            a.parse(b"1 2\n3 x\n", "snap")
        with pytest.raises(ValueError, match="nothing was parsed"):
            a.vertices()
        same(run(a, first, False), want_first)           # and it parses again after an error
        same(run(b, first, False), want_first)
    finally:
        a.close()
        b.close()
