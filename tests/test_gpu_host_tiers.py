"""Every tier edge of the host forms that share one transfer rule (vqhip_pq_encode, vqhip_tsvq_encode, the SQ / BQ maps):
the per-vector edge (8 / 9 rows; for SQ / BQ the largest count whose staging fits 64 KB and one more) and the transfer
lanes' edge (input just under and at 96 MB, with an output that makes the lanes pay).  Each call gives the same bits as
the device form on the same rows; `xfer_lane_calls` shows which calls took the lanes.  Also: host codes at an odd
address, checked against k by vqhip_pq_adc_set_codes and vqhip_pq_decode (two-byte codes, called directly: the Python
wrappers copy and check codes before the library sees them)."""
import ctypes as C

import numpy as np
import pytest

import ref_sqbq as R
from vq_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
LANES_MIN = 96 << 20  # input bytes from which a batch may take the transfer lanes
STAGE_MAX = 65536     # SQ / BQ: staging bytes of the largest per-vector call


def _edge_rows(edge: str, row_bytes: int, small: int = 8) -> int:
    return {"small": small, "small+1": small + 1, "under": LANES_MIN // row_bytes - 1, "at": LANES_MIN // row_bytes}[edge]


def _to_device(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _empty(shape, dtype):
    import torch

    return torch.empty(shape, dtype=dtype, device="cuda")


def _counted(fn):
    """fn()'s result and the number of transfer-lane calls it made"""
    before = _lib.xfer_lane_calls()
    out = fn()
    return out, _lib.xfer_lane_calls() - before


# ---- PQ: m=32, k=300 (two-byte codes), sub_dim 2: 256 B of rows, 64 B of codes and 128 B of f16 per row, so each
# output alone is at least a quarter of the input and every mode takes the lanes from 96 MB on
M, K, SD = 32, 300, 2
D = M * SD


@pytest.fixture(scope="module")
def pq():
    rng = np.random.default_rng(71)
    enc = _lib.PQEncoder(rng.standard_normal((M, K, SD)).astype(F), _lib.EUCLIDEAN)
    X = rng.standard_normal((LANES_MIN // (D * 4), D)).astype(F)
    yield enc, X
    enc.close()


def _pq_device(enc, X):
    import torch

    n = X.shape[0]
    dx, dc, df = _to_device(X), _empty((n, M), torch.int16), _empty((n, D), torch.int16)
    torch.cuda.synchronize()  # (the library launches on its own stream: torch's copy must have landed)
    enc.encode_device(dx.data_ptr(), n, dc.data_ptr(), df.data_ptr())
    _lib.synchronize()
    return dc.cpu().numpy().view(np.uint16), df.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("edge", ["small", "small+1", "under", "at"])
@pytest.mark.parametrize("mode", ["codes", "f16", "both"])
def test_pq_encode_tier_edges(pq, mode, edge):
    enc, Xall = pq
    X = Xall[:_edge_rows(edge, D * 4)]
    want_codes, want_f16 = mode != "f16", mode != "codes"
    _lib.set_profiling(True)
    try:
        (codes, f16), lanes = _counted(lambda: enc.encode(X, want_codes=want_codes, want_f16=want_f16))
        passes = _lib.profile_collect()[0]  # assignment passes of this thread: none on the per-vector path
    finally:
        _lib.set_profiling(False)
    assert lanes == (1 if edge == "at" else 0)
    if edge == "small":
        assert passes == 0
    elif edge == "small+1":
        assert passes >= 1
    ref_codes, ref_f16 = _pq_device(enc, X)
    assert (codes is not None) == want_codes and (f16 is not None) == want_f16
    if want_codes:
        assert np.array_equal(codes, ref_codes)
    if want_f16:
        assert np.array_equal(f16.view(np.uint16), ref_f16)


# ---- TSVQ: d=4, so the leaf ids (4 B per row) alone are a quarter of the rows and take the lanes as the f16 rows do
TD = 4


@pytest.fixture(scope="module")
def tsvq(oracle):
    import vq_amd as pyvq

    rng = np.random.default_rng(72)
    tree = oracle.tsvq_build(rng.standard_normal((20000, TD)).astype(F), 6)
    t = pyvq.TSVQ.from_tree(tree["centroids"], tree["left"], tree["right"], pyvq.Distance.euclidean())
    Y = rng.standard_normal((LANES_MIN // (TD * 4), TD)).astype(F)
    yield t, Y


def _tsvq_stats(t):
    scr, und = C.c_int(0), C.c_uint64(0)
    _lib.check(_lib.load().vqhip_tsvq_last_stats(t._enc.raw, C.byref(scr), C.byref(und)))
    return bool(scr.value)


def _tsvq_device(t, Y):
    import torch

    n = Y.shape[0]
    dy, dl, df = _to_device(Y), _empty((n,), torch.int32), _empty((n, TD), torch.int16)
    torch.cuda.synchronize()
    _lib.check(_lib.load().vqhip_tsvq_encode_device(t._enc.raw, C.c_void_p(dy.data_ptr()), n, C.c_void_p(dl.data_ptr()),
                                                    C.c_void_p(df.data_ptr())))
    _lib.synchronize()
    return dl.cpu().numpy(), df.cpu().numpy().view(np.uint16), _tsvq_stats(t)


@pytest.mark.parametrize("edge", ["small", "small+1", "under", "at"])
@pytest.mark.parametrize("mode", ["leaf", "f16"])
def test_tsvq_encode_tier_edges(tsvq, mode, edge):
    t, Yall = tsvq
    Y = Yall[:_edge_rows(edge, TD * 4)]
    n = Y.shape[0]
    leaf = np.empty(n, np.int32) if mode == "leaf" else None
    f16 = np.empty((n, TD), np.uint16) if mode == "f16" else None

    def host():  # directly: TSVQ's own batch methods may hand large batches to the multi-device encoder
        _lib.check(_lib.load().vqhip_tsvq_encode(t._enc.raw, _lib.ptr(Y, _lib._f32p), n, _lib.ptr(leaf, _lib._i32p),
                                                 _lib.ptr(f16, _lib._u16p)))
        return _tsvq_stats(t)

    screened, lanes = _counted(host)
    assert lanes == (1 if edge == "at" else 0)
    ref_leaf, ref_f16, dev_screened = _tsvq_device(t, Y)
    if edge == "small":
        assert not screened  # the per-vector kernel walks the tree exactly
    elif edge == "small+1":
        assert screened == dev_screened  # the one-stream pass went through the device form
    if leaf is not None:
        assert np.array_equal(leaf, ref_leaf)
    if f16 is not None:
        assert np.array_equal(f16, ref_f16)


# ---- SQ / BQ: elementwise, per-vector while input and output fit the 64 KB staging (the output 16-byte aligned)
def _largest_staged(in_sz: int, out_sz: int) -> int:
    def stage(c):
        return (c * in_sz + 15) // 16 * 16 + c * out_sz

    c = STAGE_MAX // (in_sz + out_sz)
    while stage(c + 1) <= STAGE_MAX:
        c += 1
    while stage(c) > STAGE_MAX:
        c -= 1
    return c


def _sqbq_count(edge: str, in_sz: int, out_sz: int) -> int:
    small = _largest_staged(in_sz, out_sz)
    return {"small": small, "small+1": small + 1, "under": LANES_MIN // in_sz - 1, "at": LANES_MIN // in_sz}[edge]


@pytest.fixture(scope="module")
def sqbq_inputs():
    import vq_amd

    rng = np.random.default_rng(73)
    x = rng.uniform(-1.1, 1.1, LANES_MIN // 4).astype(F)
    codes = rng.integers(0, 256, LANES_MIN, dtype=np.uint8)
    return vq_amd.ScalarQuantizer(-1.0, 1.0, 256), vq_amd.BinaryQuantizer(0.0, 2, 5), x, codes


@pytest.mark.parametrize("edge", ["small", "small+1", "under", "at"])
@pytest.mark.parametrize("op", ["sq_encode", "sq_decode", "bq_encode", "bq_decode"])
def test_sqbq_host_tier_edges(sqbq_inputs, op, edge):
    import torch

    sq, bq, xall, call = sqbq_inputs
    q = sq if op.startswith("sq") else bq
    if op.endswith("encode"):
        x = xall[:_sqbq_count(edge, 4, 1)]
        got, lanes = _counted(lambda: q.quantize_batch(x))
        dx, dc = _to_device(x), _empty(x.size, torch.uint8)
        torch.cuda.synchronize()
        q.quantize_device(dx.data_ptr(), x.size, dc.data_ptr())
        _lib.synchronize()
        ref = dc.cpu().numpy()
        cheap = (lambda: R.sq_encode(-1.0, 1.0, 256, x)) if q is sq else (lambda: R.bq_encode(0.0, 2, 5, x))
    else:
        c = call[:_sqbq_count(edge, 1, 4)]
        got, lanes = _counted(lambda: q.dequantize_batch(c))
        dc, do = _to_device(c), _empty(c.size, torch.float32)
        torch.cuda.synchronize()
        q.dequantize_device(dc.data_ptr(), c.size, do.data_ptr())
        _lib.synchronize()
        ref = do.cpu().numpy()
        cheap = (lambda: R.sq_decode(-1.0, 1.0, 256, c)) if q is sq else (lambda: R.bq_decode(0.0, 2, 5, c))
    assert lanes == (1 if edge == "at" else 0)
    assert got.dtype == ref.dtype and np.array_equal(got.view(np.uint8), ref.view(np.uint8))
    if edge.startswith("small"):
        want = cheap()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- host codes at an odd address: two-byte codes read without an aligned load, range-checked against k
def test_two_byte_host_codes_at_odd_address_are_checked():
    m, k, sd, n = 4, 300, 2, 5
    rng = np.random.default_rng(74)
    enc = _lib.PQEncoder(rng.standard_normal((m, k, sd)).astype(F), _lib.EUCLIDEAN)
    lib = _lib.load()
    raw = np.zeros(n * m * 2 + 2, np.uint8)
    off = 1 if raw.ctypes.data % 2 == 0 else 0
    ptr = C.cast(C.c_void_p(raw.ctypes.data + off), _lib._u8p)
    assert (raw.ctypes.data + off) % 2 == 1

    good = rng.integers(0, k, (n, m)).astype(np.uint16)
    raw[off:off + good.nbytes] = good.view(np.uint8).ravel()
    assert lib.vqhip_pq_adc_set_codes(enc.raw, ptr, n) == _lib.OK
    out = np.empty((n, m * sd), F)
    assert lib.vqhip_pq_decode(enc.raw, ptr, n, _lib.ptr(out, _lib._f32p)) == _lib.OK
    assert np.array_equal(out.view(np.uint32), enc.decode(good).view(np.uint32))

    bad = good.copy()
    bad[1, 3] = k  # element 7
    raw[off:off + bad.nbytes] = bad.view(np.uint8).ravel()
    assert lib.vqhip_pq_adc_set_codes(enc.raw, ptr, n) == _lib.ERR_INVALID_INPUT
    assert str(k) in _lib.last_error()
    assert lib.vqhip_pq_decode(enc.raw, ptr, n, _lib.ptr(out, _lib._f32p)) == _lib.ERR_INVALID_INPUT
    assert str(k) in _lib.last_error()
    enc.close()
