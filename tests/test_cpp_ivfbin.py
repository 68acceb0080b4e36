"""Driver of tests/cpp/test_ivfbin_hpp.cpp: vq::IVFBinaryIndex of include/vq.hpp builds with g++, reports its argument
errors and runs its host-only calls without a device, and on the GPU probes and searches as the numpy statement of
include/vqhip.h (tests/ref_ivfbin.py), from words, from codes packed on the host and from rows packed on the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_binary as B
import ref_ivfbin as R
import ref_knn as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BQ = (0.25, 3, 200)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_ivfbin") / "test_ivfbin_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ivfbin_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivfbin_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivfbin_matches_statement(exe, tmp_path):
    rng = np.random.default_rng(8)
    nlist, dim, n, nq, topk, nprobe = 40, 70, 5003, 37, 25, 6
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    rows = rng.standard_normal((n, dim)).astype(F)
    words = B.pack(rng.integers(0, 2, (n, dim)).astype(bool))
    Q = rng.standard_normal((nq, dim)).astype(F)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6Q", nlist, dim, n, nq, topk, nprobe))
        f.write(struct.pack("<fII", *BQ))
        f.write(coarse.tobytes() + lists.tobytes() + words.tobytes() + codes.tobytes() + rows.tobytes() + Q.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    a, b = n // 3, 2 * (n // 3)
    all_words = np.concatenate([words[:a], B.pack(B.bits_u8(codes[a:b], BQ[2])), B.pack(B.bits_f32(rows[b:], BQ[0]))])
    raw = np.frombuffer(open(outp, "rb").read(), np.uint32)
    W = all_words.shape[1]
    assert np.array_equal(raw[:n * W].reshape(n, W), all_words)  # packed(): add order, the quantizer's bits
    at = n * W
    for metric, cm in ((B.SQ, K.EUCLIDEAN), (B.EUC, K.MANHATTAN), (B.MAN, K.COSINE)):
        p = raw[at:at + nq * nprobe].reshape(nq, nprobe)
        at += nq * nprobe
        idx = raw[at:at + nq * topk].reshape(nq, topk)
        dist = raw[at + nq * topk:at + 2 * nq * topk].reshape(nq, topk)
        at += 2 * nq * topk
        assert np.array_equal(p, R.probe(cm, coarse, Q, nprobe))
        want = R.search(metric, cm, coarse, lists, BQ, all_words, dim, Q, nprobe, topk)
        assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1].view(np.uint32))
    assert at == raw.size
