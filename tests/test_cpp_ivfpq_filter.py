"""Driver of tests/cpp/test_ivfpq_filter_hpp.cpp: the filtered search of vq::IVFPQIndex of include/vq.hpp builds with g++,
reports its argument errors without a device, and on the GPU gives what the numpy statement of include/vqhip.h gives
(tests/ref_pq_filter.py), over plain and residual lists."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_knn as K
import ref_pq_filter as RPF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_ivfpq_filter") / "test_ivfpq_filter_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ivfpq_filter_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivfpq_filter_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivfpq_filter_matches_statement(exe, tmp_path, oracle):
    rng = np.random.default_rng(12)
    n, m, k, sd, nq, topk, nlist, nprobe = 1501, 8, 256, 2, 12, 12, 6, 2
    d = m * sd
    coarse = rng.standard_normal((nlist, d)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    lists[lists == 4] = 1  # an empty list
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    codes[n - 2:] = codes[:2]
    lists[n - 2:] = lists[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = coarse[4]
    mask = rng.random(n) < 0.2
    mask[128:448] = False
    mask[[0, 1, n - 2, n - 1]] = True, False, False, True
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<8Q", n, m, k, sd, nq, topk, nlist, nprobe))
        f.write(coarse.tobytes() + cb.tobytes() + lists.tobytes() + codes.tobytes() + Q.tobytes() + mask.astype(np.uint8).tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0
    for metric in (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN):
        for residual in (False, True):
            idx = np.frombuffer(raw, np.uint32, nq * topk, at).reshape(nq, topk)
            dist = np.frombuffer(raw, np.uint32, nq * topk, at + 4 * nq * topk).reshape(nq, topk)
            at += 8 * nq * topk
            wi, wd = RPF.ivf_search(oracle, residual, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask)
            assert np.array_equal(idx, wi), (metric, residual)
            assert np.array_equal(dist, wd.view(np.uint32)), (metric, residual)
    assert at == len(raw)
