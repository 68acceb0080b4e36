"""Driver of tests/cpp/test_sqbq_hpp.cpp: vq::ScalarQuantizer / vq::BinaryQuantizer of include/vq.hpp build with g++,
report the reference's error variants and texts without a device, and on the GPU give what the numpy restatement of
the reference (tests/ref_sqbq.py) gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_sqbq as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_sqbq") / "test_sqbq_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_sqbq_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_sqbq_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_sqbq_matches_reference_arithmetic(exe, tmp_path):
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(5000) * 0.8).astype(F)
    x[:6] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<Q", x.size))
        f.write(x.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    n = x.size
    sc = np.frombuffer(raw, np.uint8, n, 0)
    sd = np.frombuffer(raw, F, n, n)
    bc = np.frombuffer(raw, np.uint8, n, 5 * n)
    bd = np.frombuffer(raw, F, n, 6 * n)
    assert np.array_equal(sc, R.sq_encode(-1.0, 1.0, 256, x))
    assert np.array_equal(sd.view(np.uint32), R.sq_decode(-1.0, 1.0, 256, sc).view(np.uint32))
    assert np.array_equal(bc, R.bq_encode(0.0, 0, 1, x))
    assert np.array_equal(bd, R.bq_decode(0.0, 0, 1, bc))
