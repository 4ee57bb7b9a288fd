"""csrc/exchange_layout.h on the CPU: tools/exchange_layout_host_check.cpp built with a host compiler alone and run (no GPU, no
HIP), and a look through the sources: nothing outside the header knows how a slot or a late block is laid out."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphem-rapids_amd", "csrc")


def test_exchange_layout_host_check(tmp_path):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "exchange_layout_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tools", "exchange_layout_host_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "exchange_layout_host_check: ok" in run.stdout


def _code():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)


def test_the_statistics_rows_are_counted_once():
    users = [name for name, code in _code() for _ in re.finditer(r"2 \+ 2 \* gh_fix_blocks", code)]
    assert users == ["exchange_layout.h"]


def test_the_layout_is_written_by_its_setter_only():
    """The value is made in exchange_layout.h and stored by set_layout (api.hip); packed_exchange also by gh_set_packed_rows."""
    writes = []
    for name, code in _code():
        if name == "exchange_layout.h":
            continue
        writes += [(name, m.group(0)) for m in re.finditer(r"\blay\.\w+\s*=[^=]", code)]
        writes += [(name, m.group(0)) for m in re.finditer(r"\b(?:xch\.|x\.)(?:lay|packed_exchange)\s*=[^=]", code) if name != "api.hip"]
    assert writes == []
    api = dict(_code())["api.hip"]
    assert len(re.findall(r"\bx\.lay\s*=[^=]", api)) == 1 and not re.search(r"xch\.lay\s*=[^=]", api)
    # d_new and d_stats are views: assigned where the engine's own storage is allocated and in the layout setter only
    for view in ("d_new", "d_stats"):
        assert [name for name, code in _code() for _ in re.finditer(r"h->" + view + r"\s*=[^=]", code)] == ["api.hip", "api.hip"]


def test_normalise_takes_one_finish_kind():
    engine_h = dict(_code())["engine.h"]
    decl = re.search(r"gh_status gh_launch_normalise\(([^;]*)\);", engine_h).group(1)
    assert "gh_finish_kind kind" in decl and decl.count("bool") == 1   # (with_cleanup)
