"""Driver of tests/cpp/test_filter_hpp.cpp: the filtered search and range search of vq::FlatIndex and vq::ScalarIndex and
vq::pack_row_mask of include/vq.hpp build with g++, report their argument errors without a device, and on the GPU give
what the numpy statement of include/vqhip.h gives (tests/ref_filter.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_filter as RF
import ref_knn as K
import ref_range as R
import ref_sqbq as S
import ref_sqindex as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_filter") / "test_filter_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_filter_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_filter_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_filter_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(12)
    n, d, nq, topk = 1501, 21, 5, 12
    sq = (-3.0, 3.0, 256)
    X = rng.standard_normal((n, d)).astype(F)
    X[10] = 0.0
    X[n - 2:] = X[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = X[1]
    m = rng.random(n) < 0.2
    m[128:448] = False  # whole tiles skipped
    m[[0, n - 1]] = True, False
    codes = S.sq_encode(sq[0], sq[1], sq[2], X)  # the index encodes its rows by the same rule on the device
    metrics = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN, K.COSINE)
    radii = []
    for metric in metrics:
        radii.append(R.kth_distance(metric, Q, X, 25))
        radii.append(radii[-1].copy())
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<4Q", n, d, nq, topk) + struct.pack("<ffQ", sq[0], sq[1], sq[2]))
        f.write(X.tobytes() + Q.tobytes() + m.astype(np.uint8).tobytes() + np.concatenate(radii).astype(F).tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    for mi, metric in enumerate(metrics):
        for rows, rad in ((X, radii[2 * mi]), (SI.decode(sq, codes), radii[2 * mi + 1])):
            want = RF.search(metric, Q, rows, topk, m)
            idx, dist = take(np.uint32, nq * topk).reshape(nq, topk), take(np.uint32, nq * topk).reshape(nq, topk)
            assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
            wl, wi, wd = RF.range_search(metric, Q, rows, rad, m)
            lims = take(np.uint64, nq + 1)
            assert np.array_equal(lims, wl)
            assert np.array_equal(take(np.uint32, wi.size), wi) and np.array_equal(take(np.uint32, wd.size), wd.view(np.uint32))
    assert at == len(raw)
