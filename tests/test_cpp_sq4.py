"""Driver of tests/cpp/test_sq4_hpp.cpp: vq::Scalar4Index of include/vq.hpp builds with g++ -Werror, reports its argument
errors without a device, and on the GPU creates, searches, adds, removes and searches again as the numpy statement
(tests/ref_sq4.py) and as vq_amd.Scalar4Index."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_sq4 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_sq4") / "test_sq4_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_sq4_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_sq4_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_sq4_create_search_add_remove_search(exe, tmp_path):
    import vq_amd

    rng = np.random.default_rng(9)
    n, d, nq, topk, nadd = 1501, 100, 6, 40, 70
    quant = (-2.5, 2.5, 16)
    X = rng.standard_normal((n, d)).astype(F)
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    added = R.pack4(rng.integers(0, 16, (nadd, d), dtype=np.uint8))
    gone = np.unique(np.concatenate([[0, n + nadd - 1], rng.choice(n + nadd, 300, replace=False)])).astype(np.uint32)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6QffI", n, d, nq, topk, nadd, gone.size, *quant))
        f.write(X.tobytes() + Q.tobytes() + added.tobytes() + gone.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = np.frombuffer(open(outp, "rb").read(), np.uint32)
    sqz = vq_amd.ScalarQuantizer(*quant)
    words = R.pack4(sqz.quantize_batch(X))
    w = words.shape[1]
    keep = np.ones(n + nadd, bool)
    keep[gone] = False
    after = np.concatenate([words, added])[keep]
    at = 0

    def take(count):
        nonlocal at
        at += count
        return raw[at - count:at]

    for metric, name in ((1, "euclidean"), (3, "cosine")):
        assert np.array_equal(take(n * w).reshape(n, w), words)
        py = vq_amd.Scalar4Index.from_packed(words, d, sqz, vq_amd.Distance(name))
        got = (take(nq * topk).reshape(nq, topk), take(nq * topk).reshape(nq, topk))
        for want in (R.search(metric, Q, words, d, *quant, topk), py.search(Q, topk)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1].view(np.uint32))
        lo32, hi32 = take(2)
        left = int(lo32) | int(hi32) << 32
        assert left == after.shape[0]
        assert np.array_equal(take(left * w).reshape(left, w), after)
        py.add_packed(added)
        py.remove_rows(gone)
        got = (take(nq * topk).reshape(nq, topk), take(nq * topk).reshape(nq, topk))
        for want in (R.search(metric, Q, after, d, *quant, topk), py.search(Q, topk)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1].view(np.uint32))
    assert at == raw.size
