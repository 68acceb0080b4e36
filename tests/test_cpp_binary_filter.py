"""Driver of tests/cpp/test_binary_filter_hpp.cpp: the filtered search and Hamming-radius range search of vq::BinaryIndex
and vq::IVFBinaryIndex of include/vq.hpp build with g++, report their argument errors without a device, and on the GPU
give what the numpy statement gives (tests/ref_binary_filter.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_binary as B
import ref_binary_filter as S
import ref_knn as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_binary_filter") / "test_binary_filter_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_binary_filter_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_binary_filter_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_binary_filter_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(12)
    n, d, nq, topk, nlist, nprobe = 1501, 100, 5, 12, 7, 3
    bq = (0.25, 3, 200)
    X = rng.standard_normal((n, d)).astype(F)
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = X[1]
    m = rng.random(n) < 0.2
    m[128:448] = False  # whole 64-row groups skipped
    m[[0, n - 1]] = True, False
    radii = np.array([0, d // 2, d // 3, d + 3, d // 2 - 4], np.uint32)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6Q", n, d, nq, topk, nlist, nprobe) + struct.pack("<fII", *bq))
        f.write(X.tobytes() + Q.tobytes() + m.astype(np.uint8).tobytes() + radii.tobytes() + coarse.tobytes() + lists.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    words, qw = B.pack(B.bits_f32(X, bq[0])), B.pack(B.bits_f32(Q, bq[0]))
    for metric in B.METRICS:
        wants = ((S.search(qw, words, d, bq[1], bq[2], metric, topk, m), S.range_search(qw, words, d, bq[1], bq[2], metric, radii, m)),
                 (S.ivf_search(metric, K.EUCLIDEAN, coarse, lists, bq, words, d, Q, nprobe, topk, m),
                  S.ivf_range_search(metric, K.EUCLIDEAN, coarse, lists, bq, words, d, Q, nprobe, radii, m)))
        for want, (wl, wi, wd) in wants:
            idx, dist = take(np.uint32, nq * topk).reshape(nq, topk), take(np.uint32, nq * topk).reshape(nq, topk)
            assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
            lims = take(np.uint64, nq + 1)
            assert np.array_equal(lims, wl)
            assert np.array_equal(take(np.uint32, wi.size), wi) and np.array_equal(take(np.uint32, wd.size), wd.view(np.uint32))
    assert at == len(raw)
