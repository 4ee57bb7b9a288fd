"""Edge-list ingestion by the HIP kernels (device_id = 0): the checks of tests/test_datasets_cpu.py again, then what only
the device path has -- line starts on every offset of a lane's 16 bytes, of a wave and of a workgroup, lines longer than
any tile, and chunking: the same arrays whatever the budget, cuts that fall on a row's end and beside a CR LF pair, an
error's global line number from a later chunk."""
import numpy as np
import pytest

import datasets_checks as checks
import datasets_reference as ref
import graphem_rapids_amd as gra
from graphem_rapids_amd import _native

pytestmark = pytest.mark.gpu
DEV = 0
PER_BYTE = 40        # GH_INGEST_BUDGET_PER_BYTE: chunk_bytes = budget // 40


def test_reference_output_snap():
    checks.check_reference_snap(DEV)


def test_reference_output_mtx_and_edges():
    checks.check_reference_netrepo(DEV)


@pytest.mark.parametrize("name", sorted(checks.GRAMMAR))
def test_grammar(name, tmp_path):
    checks.check_grammar(name, DEV, tmp_path)


@pytest.mark.parametrize("name", sorted(checks.ERRORS))
def test_errors_name_the_first_bad_line(name):
    checks.check_error(name, DEV)


def test_mtx_header():
    checks.check_mtx_header(DEV)


def test_results():
    checks.check_results(DEV)


def test_second_parse_and_two_handles():
    checks.check_handles(DEV)


# ---- boundaries ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def boundary_text():
    """About 200 000 lines of 3 to 40 bytes (3 MB): every 7th ends in CR LF, one is a 10 000-byte comment, one row has
    5 000 blanks between its fields.  With the restatement's rows, computed once."""
    rng = np.random.default_rng(11)
    n = 200_000
    digits_a, digits_b = rng.integers(1, 10, size=n), rng.integers(1, 10, size=n)
    a = rng.integers(0, 10 ** 9, size=n) % 10 ** digits_a
    b = rng.integers(0, 10 ** 9, size=n) % 10 ** digits_b
    pad = rng.integers(0, 20, size=n)
    lines = []
    for i in range(n):
        line = "%d %d" % (a[i], b[i])
        line += (" " * int(pad[i]) + "w")[: 38 - len(line)] if pad[i] else ""
        if i == 70_001:
            line = "#" + "c" * 9_999
        if i == 130_003:
            line = "123" + " " * 2_500 + "\t" * 2_500 + "456"
        lines.append(line + ("\r\n" if i % 7 == 0 else "\n"))
    data = "".join(lines).encode()
    assert 2_500_000 < len(data) < 4_500_000 and min(map(len, lines)) <= 5 and max(map(len, lines[:70_000])) <= 40
    return data, {d: ref.parse(data, "snap", d) for d in (False, True)}


@pytest.mark.parametrize("directed", [False, True])
def test_boundaries(boundary_text, directed):
    data, want = boundary_text
    got = gra.parse_edge_list(data, "snap", directed, False, "edges", DEV)
    checks.same(got, want[directed])
    checks.same(got, gra.parse_edge_list(data, "snap", directed, False, "edges", -1))
    if directed:
        assert [123, 456] in got[1].tolist()


# ---- chunking --------------------------------------------------------------------------------------------------------

def cuts_of(data, chunk):
    """The chunk ends the header's rule gives: the last offset in (off, off + chunk] that follows a whole terminator."""
    cuts, off, n = [], 0, len(data)
    while off < n:
        if n - off <= chunk:
            end = n
        else:
            end = off + chunk
            while end > off and not (data[end - 1:end] == b"\n" or (data[end - 1:end] == b"\r" and data[end:end + 1] != b"\n")):
                end -= 1
            assert end > off                             # no line of these texts is longer than a chunk
        cuts.append(end)
        off = end
    return cuts


def budget_text(chunk):
    """Rows such that the first chunk of `chunk` bytes ends exactly with a row's terminator, and the CR LF pair of a
    later row straddles offset 2 * chunk, where a cut by offset alone would fall between CR and LF."""
    rng = np.random.default_rng(3)
    out = bytearray()

    def row(eol=b"\n", width=0):
        a, b = rng.integers(0, 500, size=2)
        body = b"%d %d" % (int(a), int(b))
        return body + b" " * max(0, width - len(body) - len(eol)) + eol
    while len(out) < chunk - 40:
        out += row()
    out += row(width=chunk - len(out))
    assert len(out) == chunk
    while len(out) < 2 * chunk - 40:
        out += row(b"\r\n" if len(out) % 3 == 0 else b"\n")
    out += row(b"\r\n", width=2 * chunk + 1 - len(out))
    assert out[2 * chunk - 1:2 * chunk + 1] == b"\r\n"
    while len(out) < 9 * chunk:
        out += row(b"\r\n" if len(out) % 5 == 0 else b"\n")
    return bytes(out)


def parse_with_budget(data, budget, directed=False):
    h = _native.EdgeListParser(DEV)
    try:
        if budget is not None:
            h.set_memory_budget(budget)
        h.parse(data, "snap", directed, "edges")
        return (h.vertices(), h.edges(False)), h.chunking()
    finally:
        h.close()


@pytest.mark.parametrize("directed", [False, True])
def test_budget_invariance(directed):
    chunk = 512
    data = budget_text(chunk)
    cuts = cuts_of(data, chunk)
    assert cuts[0] == chunk and cuts[1] < 2 * chunk - 1 and len(cuts) >= 7
    want = ref.parse(data, "snap", directed)
    whole, (_, n_chunks) = parse_with_budget(data, None, directed)
    assert n_chunks == 1
    checks.same(whole, want)
    some, (chunk_bytes, n_chunks) = parse_with_budget(data, PER_BYTE * chunk, directed)
    assert chunk_bytes == chunk and n_chunks == len(cuts) >= 7
    checks.same(some, want)
    smallest = _native.EdgeListParser.MIN_BUDGET
    many, (chunk_bytes, n_chunks) = parse_with_budget(data, smallest, directed)
    assert chunk_bytes == smallest // PER_BYTE and n_chunks == len(cuts_of(data, chunk_bytes)) > len(cuts)
    checks.same(many, want)
    for a, b in zip(whole + some, some + many):
        assert a.tobytes() == b.tobytes()


def test_error_line_number_from_the_fifth_chunk():
    chunk = 512
    data = bytearray(budget_text(chunk))
    cuts = cuts_of(bytes(data), chunk)
    starts = [0] + [i + 1 for i in range(len(data) - 1) if data[i:i + 1] == b"\n"]   # every row of this text ends in LF
    bad = []
    for k in (4, 5):                                     # a line inside the fifth chunk, one inside the sixth
        s = next(s for s in starts if cuts[k - 1] + 100 <= s < cuts[k])
        data[s:s + 1] = b"x"                             # same length: the cuts stay
        bad.append(starts.index(s) + 1)
    data = bytes(data)
    assert cuts_of(data, chunk) == cuts
    with pytest.raises(ValueError, match="^line %d: " % bad[0]):
        ref.parse(data, "snap")
    for budget in (None, PER_BYTE * chunk, _native.EdgeListParser.MIN_BUDGET):
        with pytest.raises(ValueError, match="^line %d: invalid integer 'x" % bad[0]):
            parse_with_budget(data, budget)
    with pytest.raises(ValueError, match="^line %d: " % bad[0]):
        gra.parse_edge_list(data, device_id=-1)


def test_last_byte_a_digit_at_a_chunk_end():
    chunk = 512
    data = budget_text(chunk)[:chunk]                    # ends with a terminator at exactly one chunk
    tail = b"7 8\n" * 127 + b"9 10"                      # 512 bytes, the last one a digit, no terminator
    data += tail
    assert len(data) == 2 * chunk and data[-1:] == b"0"
    for directed in (False, True):
        got, (_, n_chunks) = parse_with_budget(data, PER_BYTE * chunk, directed)
        assert n_chunks == 2
        checks.same(got, ref.parse(data, "snap", directed))
        if directed:
            assert got[1][-1].tolist() == [9, 10]


def test_text_already_on_the_device():
    import torch
    data = checks.datasets_synth.edges_text().encode()
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    h = _native.EdgeListParser(DEV)
    try:
        for budget in (0, PER_BYTE * 1000):              # chunks that begin on any offset of the 16-byte loads
            h.set_memory_budget(budget)
            h.parse_uploaded(data, buf.data_ptr(), "edges", False, "rows")
            checks.same((h.vertices(), h.edges(False)), ref.parse(data, "edges", False, False, "rows"))
        assert h.chunking()[1] > 10
    finally:
        h.close()


def test_file_to_layout(tmp_path):
    """A SNAP file on disk -> read_edge_list -> largest component -> create_graphem -> two iterations."""
    rng = np.random.default_rng(2)
    n = 3000
    ring = np.column_stack([np.arange(n), (np.arange(n) + 1) % n])            # connected
    extra = rng.integers(0, n, size=(6000, 2))
    island = np.array([[n, n + 1], [n + 1, n + 2], [n + 3, n + 3]])           # a small component and a self-loop
    rows = np.vstack([ring, extra, island]) * 3 + 11
    path = tmp_path / "graph.txt"
    path.write_text("# a graph\n" + "".join("%d\t%d\n" % (a, b) for a, b in rows), encoding="utf-8")
    vertices, edges = gra.read_edge_list(path, device_id=DEV)
    want = ref.parse(path.read_bytes(), "snap", False, True)
    checks.same((vertices, edges), want)
    adjacency = gra.largest_connected_component(edges, n=len(vertices))
    main = np.vstack([ring, extra])
    main = main[main[:, 0] != main[:, 1]]
    n_edges = len(np.unique(np.sort(main, axis=1), axis=0))
    assert adjacency.shape == (n, n) and adjacency.nnz == 2 * n_edges
    emb = gra.create_graphem(adjacency, n_components=3, backend="hip", verbose=False, seed=0)
    pos = np.asarray(emb.run_layout(num_iterations=2))
    assert emb.n == n and emb.n_edges == n_edges and pos.shape == (n, 3) and np.isfinite(pos).all()
