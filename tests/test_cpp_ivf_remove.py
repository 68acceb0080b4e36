"""Driver of tests/cpp/test_ivf_remove_hpp.cpp: the arithmetic of a removal from an inverted file
(vq_amd/csrc/ivf_remove.hpp) builds with g++ alone; the renumbering's below(i), the schedule of k_ivf_take emulated lane by
lane and its byte offsets on both sides of 2^31 and 2^32 are checked on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_ivf_remove_arithmetic(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = tmp_path / "test_ivf_remove_hpp"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "vq_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_ivf_remove_hpp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "IVF_REMOVE_OK" in r.stdout, r.stdout + r.stderr
