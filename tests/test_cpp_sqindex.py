"""Driver of tests/cpp/test_sqindex_hpp.cpp: vq::ScalarIndex of include/vq.hpp builds with g++ -Werror, reports its
argument errors without a device, and on the GPU searches and reranks as the numpy statement (tests/ref_sqindex.py)
and as vq_amd.ScalarIndex."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_sqindex as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_sqindex") / "test_sqindex_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_sqindex_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_sqindex_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_sqindex_matches_statement_and_python(exe, tmp_path):
    import vq_amd

    rng = np.random.default_rng(9)
    n, d, nq, topk, c = 3001, 77, 6, 40, 100
    sq = (-3.0, 5.0, 17)
    X = (rng.standard_normal((n, d)) * 2).astype(F)
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    cand = np.stack([rng.choice(n, c, replace=False) for _ in range(nq)]).astype(np.uint32)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5QffI", n, d, nq, topk, c, sq[0], sq[1], sq[2]))
        f.write(X.tobytes() + Q.tobytes() + cand.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    blob = open(outp, "rb").read()
    q = vq_amd.ScalarQuantizer(*sq)
    codes = q.quantize_batch(X)
    assert np.array_equal(np.frombuffer(blob[:n * d], np.uint8).reshape(n, d), codes)
    raw = np.frombuffer(blob[n * d:], np.uint32)
    at, per = 0, nq * topk
    for metric, name in ((0, "squared_euclidean"), (1, "euclidean"), (2, "manhattan"), (3, "cosine")):
        py = vq_amd.ScalarIndex.from_codes(codes, q, vq_amd.Distance(name))
        for want, other in ((R.search(metric, Q, sq, codes, topk), py.search(Q, topk)),
                            (R.rerank(metric, Q, sq, codes, cand, topk), py.rerank(Q, cand, topk))):
            for w in (want, other):
                assert np.array_equal(raw[at:at + per].reshape(nq, topk), w[0])
                assert np.array_equal(raw[at + per:at + 2 * per].reshape(nq, topk), w[1].view(np.uint32))
            at += 2 * per
    assert at == raw.size
