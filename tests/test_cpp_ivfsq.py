"""Driver of tests/cpp/test_ivfsq_hpp.cpp: vq::IVFScalarIndex of include/vq.hpp builds with g++, reports its argument
errors and runs its host-only calls without a device, and on the GPU probes and searches as the numpy statement of
include/vqhip.h (tests/ref_ivfsq.py), from codes and from rows encoded on the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_ivfsq as R
import ref_knn as K
import ref_sqbq as Q8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SQ = (-3.0, 5.0, 17)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_ivfsq") / "test_ivfsq_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ivfsq_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivfsq_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivfsq_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(8)
    nlist, dim, n, nq, topk, nprobe = 40, 19, 5003, 37, 25, 6
    coarse = rng.uniform(-3, 5, (nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    rows = rng.uniform(-4, 6, (n, dim)).astype(F)  # the second half of the index: rows encoded on the device
    Q = rng.uniform(-3, 5, (nq, dim)).astype(F)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6Q", nlist, dim, n, nq, topk, nprobe))
        f.write(struct.pack("<ffQ", *SQ))
        f.write(coarse.tobytes() + lists.tobytes() + codes.tobytes() + rows.tobytes() + Q.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    half = n // 2
    all_codes = np.concatenate([codes[:half], Q8.sq_encode(SQ[0], SQ[1], SQ[2], rows[half:])])
    raw = np.frombuffer(open(outp, "rb").read(), np.uint8)
    assert np.array_equal(raw[:n * dim].reshape(n, dim), all_codes)  # codes(): add order, the quantizer's codes
    raw = raw[n * dim:].view(np.uint32)
    at = 0
    for metric in (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN, K.COSINE):  # vq::Distance's four
        p = raw[at:at + nq * nprobe].reshape(nq, nprobe)
        at += nq * nprobe
        idx = raw[at:at + nq * topk].reshape(nq, topk)
        dist = raw[at + nq * topk:at + 2 * nq * topk].reshape(nq, topk)
        at += 2 * nq * topk
        assert np.array_equal(p, R.probe(metric, coarse, Q, nprobe))
        want = R.search(metric, coarse, lists, SQ, all_codes, Q, nprobe, topk)
        assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
