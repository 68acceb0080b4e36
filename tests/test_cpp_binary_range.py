"""Driver of tests/cpp/test_binary_range_hpp.cpp: the Hamming-radius range search of vq::BinaryIndex and
vq::IVFBinaryIndex (include/vq.hpp) builds with g++, reports its argument errors without a device, and on the GPU
returns what the numpy statement of include/vqhip.h (tests/ref_binary_range.py) does."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_binary as B
import ref_binary_range as BR
import ref_knn as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_binary_range") / "test_binary_range_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_binary_range_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_binary_range_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_binary_range_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(8)
    n, d, nq, nlist, nprobe = 3001, 70, 6, 5, 2
    thr, low, high = 0.25, 3, 200
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    X = rng.standard_normal((n, d)).astype(F)
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[1] = X[1]
    radii = np.array([30, 0, d, 0xFFFFFFFF, 26, 33], np.uint32)
    words = B.pack(B.bits_f32(X, thr))
    wants = []
    for metric in B.METRICS:
        wants.append(BR.search_rows(Q, X, thr, low, high, metric, radii))
        for p in (nprobe, nlist):
            wants.append(BR.ivf_search(metric, K.EUCLIDEAN, coarse, lists, (thr, low, high), words, d, Q, p, radii))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5Qf2I", n, d, nq, nlist, nprobe, thr, low, high))
        f.write(X.tobytes() + Q.tobytes() + coarse.tobytes() + lists.tobytes() + radii.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0
    for k, (lims, idx, dist) in enumerate(wants):
        total = int(lims[-1])
        assert total >= 2 * n + 2 or k % 3 == 1  # (the dense and the nprobe == nlist results hold every row twice)
        got_l = np.frombuffer(raw, np.uint64, nq + 1, at)
        at += 8 * (nq + 1)
        got_i = np.frombuffer(raw, np.uint32, total, at)
        at += 4 * total
        got_d = np.frombuffer(raw, np.uint32, total, at)
        at += 4 * total
        assert np.array_equal(got_l, lims) and np.array_equal(got_i, idx) and np.array_equal(got_d, dist.view(np.uint32))
    assert at == len(raw)
