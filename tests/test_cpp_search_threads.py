"""Driver of tests/cpp/test_search_threads_hpp.cpp: four std::threads call the `const` search methods of ONE vq::FlatIndex,
ONE vq::IVFFlatIndex and ONE vq::BinaryIndex of include/vq.hpp, the masked overloads among them, each thread with its own
queries, nq and topk; every thread's results are the numpy statements' (tests/ref_*.py) bit for bit.  The rows, lists, mask
and queries are those of tests/search_thread_cases.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ref_binary as B
import ref_filter as RF
import ref_ivf_filter as IVFF
import ref_ivfflat as IFL
import ref_knn as K
import search_thread_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NPROBE = 5
PER_THREAD = ((0, 1, 1), (0, 17, 10), (60, 40, 33), (0, 130, 300))  # (first query, nq, topk)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from vq_amd import _lib

    _lib.load()  # the library is built (build() / make -C vq_amd/csrc) before the suite runs
    out = tmp_path_factory.mktemp("cpp_search_threads") / "test_search_threads_hpp"
    libdir = os.path.join(ROOT, "vq_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_search_threads_hpp.cpp"), "-o", str(out), "-L", libdir, "-lvqhip",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(out)


def test_cpp_search_threads_builds(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_cpp_search_threads_match_statement(exe, tmp_path):
    d = T.base()
    X, Q, lists, coarse, m = d["rows"], d["queries"], d["lists"], d["coarse"], d["masks"]["half"]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<6Q", T.N, T.D, T.NQ, T.NLIST, NPROBE, len(PER_THREAD)))
        for per in PER_THREAD:
            f.write(struct.pack("<3Q", *per))
        f.write(X.tobytes() + Q.tobytes() + m.astype(np.uint8).tobytes() + coarse.tobytes() + lists.astype(np.uint32).tobytes())
    r = subprocess.run([exe, "run", str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RUN_OK" in r.stdout and "gfx950" in r.stdout, r.stdout + r.stderr
    raw = open(outp, "rb").read()
    at = 0

    def take(nq, topk):
        nonlocal at
        idx = np.frombuffer(raw, np.uint32, nq * topk, at).reshape(nq, topk)
        dist = np.frombuffer(raw, np.uint32, nq * topk, at + idx.nbytes).reshape(nq, topk)
        at += 2 * idx.nbytes
        return idx, dist

    for t, (q0, nq, topk) in enumerate(PER_THREAD):
        q = Q[q0:q0 + nq]
        wants = [("flat", K.search(K.EUCLIDEAN, q, X, topk)),
                 ("flat masked", RF.search(K.EUCLIDEAN, q, X, topk, m)),
                 ("ivfflat", IFL.search(K.COSINE, coarse, lists, X, q, NPROBE, topk)),
                 ("ivfflat masked", IVFF.search(K.COSINE, coarse, lists, X, q, NPROBE, topk, m)),
                 ("binary", B.search_rows(q, X, 0.0, 0, 1, B.MAN, topk))]
        for name, want in wants:
            idx, dist = take(nq, topk)
            assert np.array_equal(idx, want[0]), f"thread {t} {name}: indices"
            assert np.array_equal(dist, want[1].view(np.uint32)), f"thread {t} {name}: distances"
    assert at == len(raw)
