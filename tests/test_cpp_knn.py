"""Driver of tests/cpp/test_knn_hpp.cpp: vq::FlatIndex of include/vq.hpp builds with g++, reports its argument errors
without a device, and on the GPU searches and reranks as the numpy statement of include/vqhip.h (tests/ref_knn.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_knn as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_knn") / "test_knn_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_knn_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_knn_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_knn_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(8)
    n, d, nq, topk, c = 3001, 45, 6, 12, 200
    X = rng.standard_normal((n, d)).astype(F)
    X[10] = 0.0
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    cand = np.stack([rng.permutation(n)[:c] for _ in range(nq)]).astype(np.uint32)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5Q", n, d, nq, topk, c))
        f.write(X.tobytes() + Q.tobytes() + cand.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = np.frombuffer(open(outp, "rb").read(), np.uint32)
    per = nq * topk
    at = 0
    for metric in (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN, K.COSINE):
        for want in (K.search(metric, Q, X, topk), K.rerank(metric, Q, X, cand, topk)):
            idx, dist = raw[at:at + per].reshape(nq, topk), raw[at + per:at + 2 * per].reshape(nq, topk)
            at += 2 * per
            assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
