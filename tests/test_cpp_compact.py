"""Driver of tests/cpp/test_compact_hpp.cpp: the arithmetic of the row compaction (vq_amd/csrc/compact.hpp) builds with g++
alone; the k-th clear bit, the unit choice, the byte offsets on both sides of 2^31 and 2^32 and the schedule of
k_compact.hip, emulated lane by lane, are checked on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_compact_arithmetic(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = tmp_path / "test_compact_hpp"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "vq_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_compact_hpp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "COMPACT_OK" in r.stdout, r.stdout + r.stderr
