"""Driver of tests/cpp/test_mutate_hpp.cpp: the add and remove methods of vq::FlatIndex, vq::ScalarIndex and
vq::BinaryIndex of include/vq.hpp build with g++, report their argument errors without a device, and on the GPU give,
for one add-then-remove sequence per index, what fresh indexes over tests/ref_mutate.py's rows give."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_mutate as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_mutate") / "test_mutate_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_mutate_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_mutate_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mutate_matches_statement(exe, tmp_path):
    from vq_amd import BinaryIndex, Distance, FlatIndex, ScalarIndex, ScalarQuantizer

    rng = np.random.default_rng(31)
    n, b, d, nq, topk = 1501, 700, 21, 5, 12
    sq = (-3.0, 3.0, 256)
    X, B = rng.standard_normal((n, d)).astype(F), rng.standard_normal((b, d)).astype(F)
    Q = rng.standard_normal((nq, d)).astype(F)
    m = rng.random(n + b) < 0.3
    m[128:448] = True  # whole groups go
    m[[0, n + b - 1]] = True, False
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5Q", n, b, d, nq, topk) + struct.pack("<ffQ", *sq))
        f.write(X.tobytes() + B.tobytes() + m.astype(np.uint8).tobytes() + Q.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    R = RM.apply(X, [("add", B), ("remove", m)])
    fresh = (FlatIndex(R, Distance.cosine()), ScalarIndex(R, ScalarQuantizer(*sq)), BinaryIndex(R))
    for ix in fresh:
        assert take(np.uint64, 1)[0] == R.shape[0]
        assert np.array_equal(take(np.uint32, b), np.arange(n, n + b))
        assert np.array_equal(take(np.uint32, R.shape[0]), RM.kept(n + b, m))
        idx, dist = ix.search(Q, topk)
        assert np.array_equal(take(np.uint32, nq * topk).reshape(nq, topk), idx), type(ix).__name__
        assert np.array_equal(take(np.uint32, nq * topk).reshape(nq, topk), dist.view(np.uint32)), type(ix).__name__
    assert np.array_equal(take(np.uint8, R.shape[0] * d).reshape(-1, d), fresh[1].codes())
    assert np.array_equal(take(np.uint32, R.shape[0]).reshape(-1, 1), fresh[2].packed())
    assert at == len(raw)
