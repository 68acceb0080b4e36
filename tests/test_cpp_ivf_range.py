"""Driver of tests/cpp/test_ivf_range_hpp.cpp: the range search of vq::IVFFlatIndex and vq::IVFScalarIndex (include/vq.hpp)
builds with g++, reports its argument errors without a device, and on the GPU returns what the numpy statement of
include/vqhip.h (tests/ref_ivf_range.py) does."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_ivf_range as RR
import ref_knn as K
import ref_sqbq as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN, K.COSINE)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_ivf_range") / "test_ivf_range_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ivf_range_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivf_range_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivf_range_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(8)
    n, d, nq, nlist, nprobe = 5001, 45, 6, 7, 3
    sq = (-3.0, 3.0, 256)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist - 1, n).astype(np.uint32)  # the last list stays empty
    X = (coarse[lists] + F(0.5) * rng.standard_normal((n, d)).astype(F)).astype(F)
    X[10] = 0.0
    X[n - 2:], lists[n - 2:] = X[:2], lists[:2]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[1] = X[1]
    codes = S.sq_encode(sq[0], sq[1], sq[2], X)
    Xq = S.sq_decode(sq[0], sq[1], sq[2], codes)
    radii, wants = [], []
    for metric in METRICS:
        for rows in (X, Xq):
            r = np.array([K.distances(metric, Q[j], rows[j % 2:j % 2 + 1])[0] for j in range(nq)], F)  # ties on the boundary
            r[4] = np.inf
            r[5] = -1.0
            assert not np.isnan(r).any()
            radii.append(r)
            wants.append(RR.search(metric, coarse, lists, rows, Q, nprobe, r))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5Q2fQ", n, d, nq, nlist, nprobe, sq[0], sq[1], sq[2]))
        f.write(coarse.tobytes() + lists.tobytes() + X.tobytes() + Q.tobytes() + np.concatenate(radii).astype(F).tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0
    for lims, idx, dist in wants:
        total = int(lims[-1])
        assert total > 100 and lims[5] == lims[6]
        got_l = np.frombuffer(raw, np.uint64, nq + 1, at)
        at += 8 * (nq + 1)
        got_i = np.frombuffer(raw, np.uint32, total, at)
        at += 4 * total
        got_d = np.frombuffer(raw, np.uint32, total, at)
        at += 4 * total
        assert np.array_equal(got_l, lims) and np.array_equal(got_i, idx) and np.array_equal(got_d, dist.view(np.uint32))
    assert at == len(raw)
