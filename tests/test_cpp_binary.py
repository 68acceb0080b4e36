"""Driver of tests/cpp/test_binary_hpp.cpp: vq::BinaryIndex of include/vq.hpp builds with g++ -Werror, reports its
argument errors without a device, and on the GPU packs and searches as the numpy statement (tests/ref_binary.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_binary as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_binary") / "test_binary_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_binary_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_binary_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_binary_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(9)
    n, d, nq, topk = 3001, 77, 6, 40
    thr, low, high = 0.1, 3, 200
    X = rng.standard_normal((n, d)).astype(F)
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4QfII", n, d, nq, topk, thr, low, high))
        f.write(X.tobytes() + Q.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = np.frombuffer(open(outp, "rb").read(), np.uint32)
    words = R.pack(R.bits_f32(X, thr))
    assert np.array_equal(raw[:words.size].reshape(words.shape), words)
    at, per = words.size, nq * topk
    for metric in (R.SQ, R.EUC, R.MAN):
        idx, dist = R.search_rows(Q, X, thr, low, high, metric, topk)
        assert np.array_equal(raw[at:at + per].reshape(nq, topk), idx)
        assert np.array_equal(raw[at + per:at + 2 * per].reshape(nq, topk), dist.view(np.uint32))
        at += 2 * per
