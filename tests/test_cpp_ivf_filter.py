"""Driver of tests/cpp/test_ivf_filter_hpp.cpp: the filtered search and range search of vq::IVFFlatIndex and
vq::IVFScalarIndex of include/vq.hpp build with g++, report their argument errors without a device, and on the GPU give
what the numpy statement of include/vqhip.h gives (tests/ref_ivf_filter.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_ivf_filter as RIF
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
    out = tmp_path_factory.mktemp("cpp_ivf_filter") / "test_ivf_filter_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ivf_filter_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivf_filter_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivf_filter_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(12)
    n, d, nq, topk, nlist, nprobe = 1501, 21, 20, 12, 6, 2
    sq = (-3.0, 3.0, 256)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    lists[lists == 4] = 1  # an empty list
    X = (coarse[lists] + F(0.6) * rng.standard_normal((n, d))).astype(F)
    X[10] = 0.0
    X[n - 2:] = X[:2]
    lists[n - 2:] = lists[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[:17] = coarse[2] + F(0.05) * rng.standard_normal((17, d)).astype(F)  # 17 queries on one list: the tile kernel
    Q[0] = X[1]
    m = rng.random(n) < 0.2
    m[128:448] = False
    m[[0, n - 1]] = True, False
    codes = S.sq_encode(sq[0], sq[1], sq[2], X)
    Xd = SI.decode(sq, codes)
    metrics = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN, K.COSINE)
    radii = []
    for metric in metrics:
        radii.append(R.kth_distance(metric, Q, X[m], 25))
        radii.append(R.kth_distance(metric, Q, Xd[m], 25))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6Q", n, d, nq, topk, nlist, nprobe) + struct.pack("<ffQ", sq[0], sq[1], sq[2]))
        f.write(coarse.tobytes() + lists.tobytes() + X.tobytes() + np.ascontiguousarray(codes, np.uint8).tobytes() + Q.tobytes())
        f.write(m.astype(np.uint8).tobytes() + np.concatenate(radii).astype(F).tobytes())
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
        for rows, rad in ((X, radii[2 * mi]), (Xd, radii[2 * mi + 1])):
            want = RIF.search(metric, coarse, lists, rows, Q, nprobe, topk, m)
            idx, dist = take(np.uint32, nq * topk).reshape(nq, topk), take(np.uint32, nq * topk).reshape(nq, topk)
            assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
            wl, wi, wd = RIF.range_search(metric, coarse, lists, rows, Q, nprobe, rad, m)
            lims = take(np.uint64, nq + 1)
            assert np.array_equal(lims, wl)
            assert np.array_equal(take(np.uint32, wi.size), wi) and np.array_equal(take(np.uint32, wd.size), wd.view(np.uint32))
    assert at == len(raw)
