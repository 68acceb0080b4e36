"""Driver of tests/cpp/test_ivf_mutate_hpp.cpp: remove_rows of the four inverted-file classes of include/vq.hpp builds
with g++, reports its argument errors and removes on the host path without a device, and on the GPU gives, behind a
search and a removal on the device, what fresh indexes given the remaining rows in one add give."""
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
    out = tmp_path_factory.mktemp("cpp_ivf_mutate") / "test_ivf_mutate_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_ivf_mutate_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_ivf_mutate_validation(exe):
    r = subprocess.run([exe, "validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "VALIDATE_OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_ivf_mutate_matches_statement(exe, tmp_path):
    from vq_amd import Distance, IVFBinaryIndex, IVFFlatIndex, IVFScalarIndex, ScalarQuantizer

    rng = np.random.default_rng(41)
    n, d, nlist, nq, topk = 1501, 21, 5, 3, 4
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.choice([0, 1, 2, 4], n).astype(np.uint32)
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((nq, d)).astype(F)
    m = rng.random(n) < 0.3
    m[128:448] = True
    m[[0, n - 1]] = True
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<5Q", n, d, nlist, nq, topk))
        f.write(coarse.tobytes() + lists.tobytes() + X.tobytes() + m.astype(np.uint8).tobytes() + Q.tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    keep = RM.kept(n, m)
    fresh = (IVFFlatIndex(coarse, Distance.cosine()), IVFScalarIndex(coarse, ScalarQuantizer(-3.0, 3.0, 256)),
             IVFBinaryIndex(coarse))
    for ix in fresh:
        ix.add_rows(lists[keep], X[keep])
        assert take(np.uint64, 1)[0] == keep.shape[0]
        assert take(np.uint64, 1)[0] == 1, "the removal moved the upload counter"
        assert np.array_equal(take(np.uint32, keep.shape[0]), keep)
        idx, dist = ix.search(Q, topk, nlist)
        assert np.array_equal(take(np.uint32, nq * topk).reshape(nq, topk), idx), type(ix).__name__
        assert np.array_equal(take(np.uint32, nq * topk).reshape(nq, topk), dist.view(np.uint32)), type(ix).__name__
    assert at == len(raw)
