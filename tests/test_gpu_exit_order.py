"""What a call on a caller's stream guarantees when it returns with kernels queued (api_common.hpp, HandleSync).

`vqhip_pq_encode_device` ends in a kernel, and that kernel carries the handle's ordering event in its own dispatch:
nothing is recorded behind it.  Both guarantees of the recorded event must hold for the carried one:
  * a later call on another stream waits for this call's work (two encodes into overlapping rows of one buffer: the
    later, 4000 times shorter one would finish first and be overwritten without the wait);
  * the caller may destroy their stream once it has run dry.
One encoder, two streams, the calls made from one thread and from two."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from vq_amd import _lib

pytestmark = pytest.mark.gpu
N, D, M, K, SHORT, REPEATS = 1_000_000, 128, 8, 256, 64, 20


def _hip_runtime():
    """the HIP runtime this process already runs on (torch's), by the path it was loaded from"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


class OwnedStream:
    """a HIP stream this test creates and really destroys (torch's streams come from a pool and never are)"""

    def __init__(self, hip):
        self.hip, self.ptr = hip, C.c_void_p()
        assert hip.hipStreamCreate(C.byref(self.ptr)) == 0

    def synchronize(self):
        assert self.hip.hipStreamSynchronize(self.ptr) == 0

    def destroy(self):
        assert self.hip.hipStreamDestroy(self.ptr) == 0
        self.ptr = None


@pytest.fixture(scope="module")
def setup():
    _lib.load()
    _lib.set_stream(None)
    _lib.set_profiling(False)
    rng = np.random.default_rng(9)
    long_rows = _lib.Dataset.synthetic(N, D, 31, 0)
    short_rows = _lib.Dataset.synthetic(SHORT, D, 32, 0)
    enc = _lib.PQEncoder(rng.random((M, K, D // M), dtype=np.float32), _lib.SQUARED_EUCLIDEAN)
    want = torch.zeros((N, M), dtype=torch.uint8, device="cuda")
    want_short = torch.zeros((SHORT, M), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    enc.encode_device(long_rows.device_ptr, N, want.data_ptr(), None)
    enc.encode_device(short_rows.device_ptr, SHORT, want_short.data_ptr(), None)
    _lib.synchronize()
    assert not torch.equal(want[:SHORT], want_short)
    want[:SHORT] = want_short  # what the buffer holds when the short call ran behind the long one
    torch.cuda.synchronize()
    yield enc, long_rows, short_rows, want
    _lib.set_stream(None)
    enc.close()
    long_rows.close()
    short_rows.close()


class Callers:
    """runs the call on stream A and the call on stream B: on the calling thread, or each on a thread of its own"""

    def __init__(self, threads):
        self.pools = [ThreadPoolExecutor(1), ThreadPoolExecutor(1)] if threads else None

    def call(self, which, fn):
        if self.pools is None:
            return fn()
        return self.pools[which].submit(fn).result()

    def close(self):
        for p in self.pools or []:
            p.shutdown()


def _encode_on(enc, stream_ptr, rows, n, codes):
    _lib.set_device(0)
    _lib.set_stream(stream_ptr)
    stale = _lib.last_error()  # the message is per thread and never cleared: empty on a fresh thread
    enc.encode_device(rows.device_ptr, n, codes.data_ptr(), None)
    assert _lib.last_error() == stale


@pytest.mark.parametrize("threads", [False, True], ids=["one_thread", "two_threads"])
def test_later_call_on_another_stream_waits(setup, threads):
    enc, long_rows, short_rows, want = setup
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    codes = torch.zeros((N, M), dtype=torch.uint8, device="cuda")
    callers = Callers(threads)
    wrong = 0
    try:
        for _ in range(REPEATS):
            codes.zero_()
            torch.cuda.synchronize()
            callers.call(0, lambda: _encode_on(enc, a.cuda_stream, long_rows, N, codes))
            callers.call(1, lambda: _encode_on(enc, b.cuda_stream, short_rows, SHORT, codes))
            a.synchronize()
            b.synchronize()
            wrong += 0 if torch.equal(codes, want) else 1
    finally:
        callers.close()
        _lib.set_stream(None)
    assert wrong == 0, f"{wrong} of {REPEATS} repeats lost the order"


@pytest.mark.parametrize("threads", [False, True], ids=["one_thread", "two_threads"])
def test_stream_destroyed_before_the_next_call(setup, threads):
    enc, long_rows, short_rows, want = setup
    hip = _hip_runtime()
    b = torch.cuda.Stream()
    codes = torch.zeros((N, M), dtype=torch.uint8, device="cuda")
    callers = Callers(threads)
    try:
        for _ in range(3):
            codes.zero_()
            torch.cuda.synchronize()
            a = OwnedStream(hip)
            callers.call(0, lambda: _encode_on(enc, a.ptr.value, long_rows, N, codes))
            a.synchronize()
            callers.call(0, lambda: _lib.set_stream(None))
            a.destroy()
            callers.call(1, lambda: _encode_on(enc, b.cuda_stream, short_rows, SHORT, codes))
            b.synchronize()
            assert torch.equal(codes, want)
    finally:
        callers.close()
        _lib.set_stream(None)


TN, TD = 1_000_000, 32


def _tsvq_on(t, stream_ptr, rows, n, leaf):
    _lib.set_device(0)
    _lib.set_stream(stream_ptr)
    _lib.check(_lib.load().vqhip_tsvq_encode_device(t._enc.raw, C.c_void_p(rows.data_ptr()), n, C.c_void_p(leaf.data_ptr()),
                                                    None))


@pytest.mark.parametrize("threads", [False, True], ids=["one_thread", "two_threads"])
def test_tsvq_later_call_on_another_stream_waits(oracle, threads):
    """the screened descent's last kernel carries the tree's ordering event in the same way"""
    import vq_amd as pyvq

    rng = np.random.default_rng(73)
    tree = oracle.tsvq_build(rng.random((20000, TD), dtype=np.float32), 6)
    t = pyvq.TSVQ.from_tree(tree["centroids"], tree["left"], tree["right"], pyvq.Distance.squared_euclidean())
    _lib.set_stream(None)
    gen = torch.Generator(device="cuda").manual_seed(5)
    long_rows = torch.rand((TN, TD), generator=gen, device="cuda")
    short_rows = torch.rand((SHORT, TD), generator=gen, device="cuda")
    want = torch.full((TN,), -1, dtype=torch.int32, device="cuda")
    want_short = torch.full((SHORT,), -1, dtype=torch.int32, device="cuda")
    leaf = torch.empty((TN,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _tsvq_on(t, None, long_rows, TN, want)
    _tsvq_on(t, None, short_rows, SHORT, want_short)
    _lib.synchronize()
    assert not torch.equal(want[:SHORT], want_short)
    want[:SHORT] = want_short
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    callers = Callers(threads)
    wrong = 0
    try:
        for _ in range(REPEATS):
            leaf.fill_(-1)
            torch.cuda.synchronize()
            callers.call(0, lambda: _tsvq_on(t, a.cuda_stream, long_rows, TN, leaf))
            callers.call(1, lambda: _tsvq_on(t, b.cuda_stream, short_rows, SHORT, leaf))
            a.synchronize()
            b.synchronize()
            wrong += 0 if torch.equal(leaf, want) else 1
    finally:
        callers.close()
        _lib.set_stream(None)
    assert wrong == 0, f"{wrong} of {REPEATS} repeats lost the order"
