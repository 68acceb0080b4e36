"""Driver of tests/cpp/test_ivfsq4_hpp.cpp: vq::IVFScalar4Index of include/vq.hpp builds with g++ (-Wall -Wextra -Werror),
reports its argument errors and runs its host-only calls without a device; nib_word_offset holds at the list-order rows
the inverted-file kernels hand it on both sides of bytes 2^31 and 2^32; and on the GPU the class creates, adds (codes, packed
words and rows encoded on the device), searches, removes and searches as the numpy statement of include/vqhip.h
(tests/ref_ivfsq4.py) -- the C++ side compares the same calls with vq::IVFScalarIndex."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_ivfsq4 as R
import ref_knn as K
import ref_sqbq as Q8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SQ = (-1.0, 1.0, 16)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_ivfsq4") / "test_ivfsq4_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "vq_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_ivfsq4_hpp.cpp"), "-o", str(out),
           "-L", libdir, "-lvqhip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivfsq4_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


def test_cpp_ivfsq4_word_offsets_of_list_order_rows(exe):
    r = subprocess.run([exe, "offsets"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OFFSETS_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivfsq4_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(8)
    nlist, dim, n, nq, topk, nprobe = 7, 19, 1501, 37, 25, 3
    coarse = rng.uniform(-1, 1, (nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 16, (n, dim)).astype(np.uint8)
    rows = rng.uniform(-1.5, 1.5, (n, dim)).astype(F)  # the last third of the index: rows encoded on the device
    Q = rng.uniform(-1, 1, (nq, dim)).astype(F)
    remove = rng.random(n) < 0.3
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6Q", nlist, dim, n, nq, topk, nprobe))
        f.write(struct.pack("<ffQ", *SQ))
        f.write(coarse.tobytes() + lists.tobytes() + codes.tobytes() + rows.tobytes() + Q.tobytes() + remove.astype(np.uint8).tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    b = 2 * n // 3
    all_codes = np.concatenate([codes[:b], Q8.sq_encode(SQ[0], SQ[1], SQ[2], rows[b:])])
    raw = np.frombuffer(open(outp, "rb").read(), np.uint8)
    assert np.array_equal(raw[:n * dim].reshape(n, dim), all_codes)  # codes(): add order, the quantizer's codes
    raw = raw[n * dim:].view(np.uint32)
    kept = np.flatnonzero(~remove)
    at = 0

    def take(count, shape):
        nonlocal at
        a = raw[at:at + count].reshape(shape)
        at += count
        return a

    for metric in (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN, K.COSINE):  # vq::Distance's four
        p = take(nq * nprobe, (nq, nprobe))
        assert np.array_equal(p, R.probe(metric, coarse, Q, nprobe))
        for l, c in ((lists, all_codes), (lists[kept], all_codes[kept])):  # before and after the removal
            idx, dist = take(nq * topk, (nq, topk)), take(nq * topk, (nq, topk))
            want = R.search(metric, coarse, l, SQ, c, Q, nprobe, topk)
            assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
    assert at == raw.size
