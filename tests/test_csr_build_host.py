"""csrc/csr_build.h on the CPU: tools/csr_build_host_check.cpp built with a host compiler alone and run (no GPU, no HIP)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csr_build_host_check(tmp_path):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "csr_build_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "csr_build_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "csr_build_host_check: ok" in run.stdout
