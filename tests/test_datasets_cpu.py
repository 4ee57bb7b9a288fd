"""Edge-list ingestion on the library's host path (device_id = -1) and the dataset catalogue, without a GPU: the
reference's own output bit for bit, the grammar of include/graphem_hip.h case by case against its Python restatement,
the errors with their line numbers, and load_dataset's name resolution and file handling with the network shut."""
import ast
import gzip
import os
import socket

import numpy as np
import pytest

import datasets_checks as checks
import datasets_reference as ref
import datasets_synth
import graphem_rapids_amd as gra
from conftest import load_golden
from graphem_rapids_amd import _native, datasets

HOST = -1
INGEST_SYMBOLS = ["gh_ingest_create", "gh_ingest_destroy", "gh_ingest_last_error", "gh_ingest_set_memory_budget",
                  "gh_ingest_parse", "gh_ingest_parse_uploaded", "gh_ingest_counts", "gh_ingest_chunking",
                  "gh_ingest_copy_vertices", "gh_ingest_copy_edges"]


def test_symbols_are_bound_and_exported():
    lib = _native.load()
    for name in INGEST_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.SYMBOLS, name
    for name in ("load_dataset", "read_edge_list", "list_available_datasets", "load_dataset_as_networkx",
                 "load_dataset_adjacency", "get_data_directory", "SNAPDataset", "NetworkRepositoryDataset",
                 "SemanticScholarDataset"):
        assert name in gra.__all__ and hasattr(gra, name), name


def test_reference_output_snap():
    checks.check_reference_snap(HOST)


def test_reference_output_mtx_and_edges():
    checks.check_reference_netrepo(HOST)


@pytest.mark.parametrize("name", sorted(checks.GRAMMAR))
def test_grammar(name, tmp_path):
    checks.check_grammar(name, HOST, tmp_path)


@pytest.mark.parametrize("name", sorted(checks.ERRORS))
def test_errors_name_the_first_bad_line(name):
    checks.check_error(name, HOST)


def test_mtx_header():
    checks.check_mtx_header(HOST)


def test_results():
    checks.check_results(HOST)


def test_second_parse_and_two_handles():
    checks.check_handles(HOST)


def test_handle_refuses_bad_arguments():
    h = _native.EdgeListParser(HOST)
    with pytest.raises(ValueError, match="format must be"):
        h.parse(b"1 2", "csv")
    with pytest.raises(ValueError, match="vertices_from must be"):
        h.parse(b"1 2", "snap", False, "files")
    with pytest.raises(ValueError, match="at least 4096"):
        h.set_memory_budget(_native.EdgeListParser.MIN_BUDGET - 1)
    with pytest.raises(ValueError, match="budget must be >= 0"):
        h.set_memory_budget(-1)
    h.set_memory_budget(_native.EdgeListParser.MIN_BUDGET)
    h.set_memory_budget(0)
    h.parse(b"1 2", "snap")
    assert h.chunking()[1] == 0 and (h.rows, h.n_edges, h.n_vertices) == (1, 1, 2)
    h.close()
    with pytest.raises(ValueError, match="handle is NULL"):
        h.parse(b"1 2", "snap")


# ---- the catalogue: every test below runs with the network shut ------------------------------------------------------

@pytest.fixture
def no_network(monkeypatch):
    def refuse(*args, **kwargs):
        pytest.fail("the datasets module tried to open a connection")
    monkeypatch.setattr(socket.socket, "connect", refuse)
    monkeypatch.setattr(socket.socket, "connect_ex", refuse)
    monkeypatch.delenv("GRAPHEM_DATA_DIR", raising=False)


def test_module_names_no_networking_import(no_network):
    with open(datasets.__file__, encoding="utf-8") as fh:
        tree = ast.parse(fh.read())
    named = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            named.update(alias.name.split(".")[0] for alias in node.names)
        elif isinstance(node, ast.ImportFrom) and node.module:
            named.add(node.module.split(".")[0])
    assert not named & {"requests", "urllib", "urllib3", "http", "socket", "ftplib", "aiohttp", "httpx"}, named


def test_name_resolution_and_messages(no_network, tmp_path):
    snap = ", ".join(datasets.SNAPDataset.AVAILABLE_DATASETS)
    for name, cls in (("snap-ca-GrQc", datasets.SNAPDataset), ("ca-GrQc", datasets.SNAPDataset),
                      ("netrepo-ia-reality", datasets.NetworkRepositoryDataset), ("ia-reality", datasets.NetworkRepositoryDataset),
                      ("semanticscholar-s2-CS", datasets.SemanticScholarDataset), ("s2-CS", datasets.SemanticScholarDataset)):
        loader = datasets._loader(name, tmp_path)   # pylint: disable=protected-access
        assert type(loader) is cls and loader.data_dir == tmp_path / loader.name
    with pytest.raises(ValueError, match=r"^Unknown dataset: nothing$"):
        gra.load_dataset("nothing", tmp_path)
    with pytest.raises(ValueError) as info:
        gra.load_dataset("snap-nothing", tmp_path)
    assert str(info.value) == f"Unknown SNAP dataset: nothing. Available datasets: {snap}"
    with pytest.raises(ValueError, match=r"^Unknown Network Repository dataset: x\. Available datasets: soc-hamsterster, socfb-MIT, "):
        gra.load_dataset("netrepo-x", tmp_path)
    with pytest.raises(ValueError, match=r"^Unknown Semantic Scholar dataset: y\. Available datasets: s2-CS$"):
        gra.load_dataset("semanticscholar-y", tmp_path)
    assert not any(tmp_path.iterdir())              # no directory was created


def test_list_available_datasets(no_network):
    listed = gra.list_available_datasets()
    assert list(listed) == ["snap-facebook_combined", "snap-ego-twitter", "snap-wiki-vote", "snap-ca-GrQc", "snap-ca-HepTh",
                            "snap-oregon1_010331", "snap-p2p-Gnutella04", "snap-email-Enron", "netrepo-soc-hamsterster",
                            "netrepo-socfb-MIT", "netrepo-ca-cit-HepPh", "netrepo-web-google-dir", "netrepo-ia-reality",
                            "semanticscholar-s2-CS"]
    assert listed["snap-ego-twitter"] == {"source": "SNAP", "name": "ego-twitter", "description": "Twitter ego network",
                                          "nodes": 81306, "edges": 1768149, "directed": True}
    assert listed["netrepo-web-google-dir"] == {"source": "Network Repository", "name": "web-google-dir",
                                                "description": "Google web graph", "directed": True}
    assert listed["semanticscholar-s2-CS"] == {"source": "Semantic Scholar", "name": "s2-CS",
                                               "description": "Computer Science citation network from Semantic Scholar"}
    assert datasets.SNAPDataset.AVAILABLE_DATASETS["wiki-vote"]["url"] == "https://snap.stanford.edu/data/wiki-Vote.txt.gz"
    assert datasets.NetworkRepositoryDataset.AVAILABLE_DATASETS["ca-cit-HepPh"] == {
        "url": "https://nrvis.com/download/data/ca/ca-cit-HepPh.zip", "description": "Citation network of Arxiv High Energy Physics",
        "directed": True, "file_pattern": "ca-cit-HepPh.mtx"}


def test_missing_file_names_path_and_url(no_network, tmp_path, monkeypatch):
    with pytest.raises(FileNotFoundError) as info:
        gra.load_dataset("snap-ca-GrQc", tmp_path)
    assert str(tmp_path / "snap-ca-GrQc" / "ca-GrQc.txt") in str(info.value)
    assert "https://snap.stanford.edu/data/ca-GrQc.txt.gz" in str(info.value)
    with pytest.raises(FileNotFoundError) as info:
        gra.load_dataset("s2-CS", tmp_path)
    assert "s2-CS-nodes.csv" in str(info.value) and "s2-CS.tar.gz" in str(info.value)
    loader = datasets.SNAPDataset("ca-GrQc", tmp_path)
    assert not loader.is_downloaded()
    with pytest.raises(RuntimeError) as info:
        loader.download()
    assert loader.url in str(info.value) and str(loader.expected_path()) in str(info.value)
    for cls, name in ((datasets.NetworkRepositoryDataset, "ia-reality"), (datasets.SemanticScholarDataset, "s2-CS")):
        with pytest.raises(RuntimeError, match="downloads nothing"):
            cls(name, tmp_path).download()
    assert not any(tmp_path.iterdir())
    monkeypatch.setenv("GRAPHEM_DATA_DIR", str(tmp_path / "elsewhere"))
    assert gra.get_data_directory() == tmp_path / "elsewhere" and not (tmp_path / "elsewhere").exists()
    monkeypatch.delenv("GRAPHEM_DATA_DIR")
    assert str(gra.get_data_directory()) == os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(datasets.__file__))), "data")


def test_snap_dataset_plain_and_gz(no_network, tmp_path, capsys):
    text = b"# Directed graph\n# FromNodeId\tToNodeId\n30\t10\n10\t30\n10\t20 7\n20\t20\n40\t10\n"
    folder = tmp_path / "snap-wiki-vote"
    folder.mkdir()
    (folder / "wiki-Vote.txt").write_bytes(text)
    plain = gra.load_dataset("snap-wiki-vote", tmp_path)                  # directed in the catalogue
    checks.same(plain, ([10, 20, 30, 40], [[30, 10], [10, 30], [10, 20], [20, 20], [40, 10]]))
    checks.same(gra.load_dataset("wiki-vote", tmp_path, relabel=True), ([0, 1, 2, 3], [[2, 0], [0, 2], [0, 1], [1, 1], [3, 0]]))
    (folder / "wiki-Vote.txt").unlink()
    with gzip.open(folder / "wiki-Vote.txt.gz", "wb") as fh:
        fh.write(text)
    checks.same(gra.load_dataset("snap-wiki-vote", tmp_path), plain)      # .gz beside no .txt
    assert datasets.SNAPDataset("wiki-vote", tmp_path).is_downloaded()
    adjacency = gra.load_dataset_adjacency("wiki-vote", tmp_path)
    assert adjacency.shape == (4, 4) and (adjacency != adjacency.T).nnz == 0 and adjacency.diagonal().sum() == 0
    assert sorted(zip(*adjacency.nonzero())) == [(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)] and set(adjacency.data) == {1}
    # an undirected catalogue entry: vertices from the returned edges
    folder = tmp_path / "snap-ca-GrQc"
    folder.mkdir()
    (folder / "ca-GrQc.txt").write_bytes(text)
    checks.same(gra.load_dataset("ca-GrQc", tmp_path), ([10, 20, 30, 40], [[10, 20], [10, 30], [10, 40]]))
    (folder / "ca-GrQc.txt").write_bytes(b"7 7\n1 2\n")
    checks.same(gra.load_dataset("ca-GrQc", tmp_path), ([1, 2], [[1, 2]]))
    graph = gra.load_dataset_as_networkx("ca-GrQc", tmp_path)
    assert sorted(graph.nodes) == [0, 1] and sorted(graph.edges) == [(0, 1)]
    datasets.SNAPDataset("ca-GrQc", tmp_path).info()
    assert "Number of vertices: 2" in capsys.readouterr().out


def test_network_repository_files(no_network, tmp_path):
    gold = load_golden("datasets_ref")
    with pytest.raises(FileNotFoundError) as info:
        gra.load_dataset("netrepo-ia-reality", tmp_path)
    assert "ia-reality.mtx" in str(info.value) and "https://nrvis.com/download/data/ia/ia-reality.zip" in str(info.value)
    nested = tmp_path / "netrepo-ia-reality" / "unpacked"
    nested.mkdir(parents=True)
    (nested / "ia-reality.mtx").write_text(datasets_synth.mtx_text(), encoding="utf-8")
    checks.same(gra.load_dataset("ia-reality", tmp_path), (gold["mtx_undirected_vertices"], gold["mtx_undirected_edges"]))
    (tmp_path / "netrepo-ia-reality" / "ia-reality.mtx").write_text("%\n1 1 0\n", encoding="utf-8")
    with pytest.raises(RuntimeError, match="Multiple files matched ia-reality.mtx"):
        gra.load_dataset("ia-reality", tmp_path)
    folder = tmp_path / "netrepo-web-google-dir"
    folder.mkdir()
    (folder / "web-google-dir.edges").write_text(datasets_synth.edges_text(), encoding="utf-8")
    checks.same(gra.load_dataset("netrepo-web-google-dir", tmp_path), (gold["edges_directed_vertices"], gold["edges_directed_edges"]))
    # 'rows': a vertex that has only a self-loop stays
    (folder / "web-google-dir.edges").write_text("9 9\n1 2\n", encoding="utf-8")
    checks.same(gra.load_dataset("web-google-dir", tmp_path), ([1, 2, 9], [[9, 9], [1, 2]]))


def test_semantic_scholar_reference_output(no_network, tmp_path):
    gold = load_golden("datasets_ref")
    nodes, cites = datasets_synth.s2_csvs()
    assert datasets_synth.text_sha1(nodes + cites) == str(gold["s2_text_sha1"])
    folder = tmp_path / "semanticscholar-s2-CS"
    folder.mkdir()
    (folder / "s2-CS-nodes.csv").write_text(nodes, encoding="utf-8")
    (folder / "s2-CS-citations.csv").write_text(cites, encoding="utf-8")
    got = gra.load_dataset("semanticscholar-s2-CS", tmp_path)
    checks.same(got, (gold["s2_vertices"], gold["s2_edges"]))
    ranks, rel = gra.load_dataset("s2-CS", tmp_path, relabel=True)
    assert np.array_equal(got[0][rel], got[1]) and np.array_equal(ranks, np.arange(len(got[0])))


def test_read_edge_list_formats_by_suffix(no_network, tmp_path):
    mtx = b"%%MatrixMarket matrix\n3 3 2\n1 2\n3 1\n"
    for name, fmt in (("a.mtx", "mtx"), ("a.edges", "edges"), ("a.txt", "snap"), ("a", "snap"), ("a.mtx.gz", "mtx")):
        path = tmp_path / name
        if name.endswith(".gz"):
            with gzip.open(path, "wb") as fh:
                fh.write(mtx)
        else:
            path.write_bytes(mtx)
        if fmt == "mtx":
            checks.same(gra.read_edge_list(path, relabel=False, device_id=HOST), ([0, 1, 2], [[0, 1], [0, 2]]))
        else:
            with pytest.raises(ValueError, match="^line 1: invalid integer '%%MatrixMarket'"):
                gra.read_edge_list(tmp_path / name, device_id=HOST)
    checks.same(gra.read_edge_list(tmp_path / "a.txt", format="mtx", relabel=False, device_id=HOST), ref.parse(mtx, "mtx"))
