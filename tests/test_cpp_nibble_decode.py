"""Driver of tests/cpp/test_nibble_decode_hpp.cpp: the host-and-device part of vq_amd/csrc/nibble_decode.hpp builds with
g++ alone; the nibble extraction, the decode rule, the lane schedule of a chunk's fill emulated lane by lane, the LDS
banks of every wave store and the word offsets on both sides of 2^31 and 2^32 bytes are checked on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_nibble_decode_arithmetic(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = tmp_path / "test_nibble_decode_hpp"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "vq_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_nibble_decode_hpp.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "NIBBLE_DECODE_OK" in r.stdout, r.stdout + r.stderr
