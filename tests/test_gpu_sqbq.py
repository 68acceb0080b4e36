"""ScalarQuantizer / BinaryQuantizer on the MI355X (vqhip_sq_* / vqhip_bq_*, vq_amd/csrc/k_sqbq.hip) against the numpy
restatement of the reference (tests/ref_sqbq.py), bit for bit: every threshold +-4 ulps, the special values, 2^24
patterns strided over the whole f32 space, all 256 codes on decode; host and device forms; unaligned device pointers
and counts around the kernels' 16-element runs; one 1M x 384 batch; the per-vector calls; the reference's known
answers (tests/golden/sqbq_kat.json); the eval CLI."""
import json
import os

import numpy as np
import pytest

import ref_sqbq as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

SPECIAL_BITS = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,              # +-0, +-inf
    0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0xFFFFFFFF,  # NaNs with payloads, quiet and signalling
    0x7FA5A5A5, 0xFF812345,
    0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000,  # subnormals
    0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,              # smallest normal, largest finite
], dtype=np.uint32)


def ulps_around(vals, k=4) -> np.ndarray:
    """every finite value of `vals` and its k neighbours each way"""
    v = np.asarray(vals, F)
    v = v[np.isfinite(v)]
    out = [v]
    up, dn = v.copy(), v.copy()
    for _ in range(k):
        up, dn = R.nextafter32(up, np.inf), R.nextafter32(dn, -np.inf)
        out += [up, dn]
    return np.concatenate(out).astype(F)


def strided_patterns() -> np.ndarray:
    return (np.arange(1 << 24, dtype=np.uint64) * 256 + 0x5B).astype(np.uint32).view(F)


def sq_inputs(sq) -> np.ndarray:
    b = sq.thresholds()
    return np.concatenate([ulps_around(b[1:]), ulps_around([sq.min, sq.max]), SPECIAL_BITS.view(F),
                           strided_patterns()]).astype(F)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def device_encode(q, x: np.ndarray) -> np.ndarray:
    import torch

    from vq_amd import _lib

    dx = torch.from_numpy(x).cuda()
    dc = torch.empty(x.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the library launches on its own stream: torch's copy must have landed)
    q.quantize_device(dx.data_ptr(), x.size, dc.data_ptr())
    _lib.synchronize()
    return dc.cpu().numpy()


def device_decode(q, c: np.ndarray) -> np.ndarray:
    import torch

    from vq_amd import _lib

    dc = torch.from_numpy(c).cuda()
    do = torch.empty(c.size, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    q.dequantize_device(dc.data_ptr(), c.size, do.data_ptr())
    _lib.synchronize()
    return do.cpu().numpy()


@pytest.mark.parametrize("cfg", R.SQ_CONFIGS, ids=[f"{a:g},{b:g},{c}" for a, b, c in R.SQ_CONFIGS])
def test_sq_encode_decode_exact(cfg):
    import vq_amd

    sq = vq_amd.ScalarQuantizer(*cfg)
    assert sq.step == float(R.sq_step(*cfg)) or (np.isnan(sq.step) and np.isnan(R.sq_step(*cfg)))
    x = sq_inputs(sq)
    want = R.sq_encode(*cfg, x)
    host = sq.quantize_batch(x)
    bad = np.flatnonzero(host != want)
    assert bad.size == 0, f"{bad.size} mismatches, first x={x[bad[0]]!r} ({x[bad[0]:bad[0]+1].view(np.uint32)[0]:#010x}) got {host[bad[0]]} want {want[bad[0]]}"
    assert np.array_equal(device_encode(sq, x), want)
    codes = np.arange(256, dtype=np.uint8)
    want_d = R.sq_decode(*cfg, codes)
    assert same_bits(sq.dequantize_batch(codes), want_d)
    assert same_bits(device_decode(sq, codes), want_d)


def test_sq_degenerate_steps_known_answers():
    import vq_amd

    inf_step = vq_amd.ScalarQuantizer(-3e38, 3e38, 256)
    assert np.isinf(inf_step.step)
    got = inf_step.quantize_batch(np.array([-3e38, 0.0, 3e38, np.inf, np.nan], F))
    assert got.tolist() == [0, 0, 0, 0, 0]  # x = max: inf / inf = NaN -> 0
    zero_step = vq_amd.ScalarQuantizer(0.0, 1e-45, 3)
    assert zero_step.step == 0.0
    got = zero_step.quantize_batch(np.array([0.0, -1.0, 1e-45, 1.0, np.nan], F))
    assert got.tolist() == [0, 0, 2, 2, 0]  # x = min: 0 / 0 = NaN -> 0; above min: +inf -> levels - 1


def test_bq_encode_decode_exact():
    import vq_amd

    strided = strided_patterns()
    for thr in (0.0, -0.0, 0.5, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1e-40, 123.456):
        for low, high in ((0, 1), (0, 255), (254, 255), (7, 200), (0, 2)):
            bq = vq_amd.BinaryQuantizer(thr, low, high)
            x = np.concatenate([ulps_around([thr, 0.0]), np.array([-0.0, 0.0], F), SPECIAL_BITS.view(F)])
            if (low, high) == (0, 1):
                x = np.concatenate([x, strided])
            want = R.bq_encode(thr, low, high, x)
            assert np.array_equal(bq.quantize_batch(x), want), (thr, low, high)
            assert np.array_equal(device_encode(bq, x), want), (thr, low, high)
            codes = np.arange(256, dtype=np.uint8)
            want_d = R.bq_decode(thr, low, high, codes)
            assert same_bits(bq.dequantize_batch(codes), want_d)
            assert same_bits(device_decode(bq, codes), want_d)
    # -0.0 and +0.0 are one threshold: both sides of the comparison
    assert vq_amd.BinaryQuantizer(-0.0).quantize(np.array([0.0, -0.0, -1e-45], F)).tolist() == [1, 1, 0]
    assert vq_amd.BinaryQuantizer(0.0).quantize(np.array([0.0, -0.0, -1e-45], F)).tolist() == [1, 1, 0]


COUNTS = sorted({c for m in (16, 64, 256, 1024, 4096) for c in (m - 1, m, m + 1)} | {0, 1, 2, 3, 31, 33, 4099})


@pytest.mark.parametrize("kind", ["sq", "sq_direct_inf", "bq"])
def test_device_forms_unaligned_pointers_and_counts(kind):
    """pointer offsets 0..15 elements on the f32 side and 0..15 bytes on the code side, counts around the 16-element
    runs; the bytes / floats around each output stay untouched"""
    import torch

    import vq_amd
    from vq_amd import _lib

    q = {"sq": lambda: vq_amd.ScalarQuantizer(-1.0, 1.0, 256), "sq_direct_inf": lambda: vq_amd.ScalarQuantizer(-3e38, 3e38, 256),
         "bq": lambda: vq_amd.BinaryQuantizer(0.25, 3, 9)}[kind]()
    ref_e = (lambda x: R.sq_encode(q.min, q.max, q.levels, x)) if kind != "bq" else (lambda x: R.bq_encode(0.25, 3, 9, x))
    ref_d = (lambda c: R.sq_decode(q.min, q.max, q.levels, c)) if kind != "bq" else (lambda c: R.bq_decode(0.25, 3, 9, c))
    nmax = max(COUNTS)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(nmax + 16) * 0.7).astype(F)
    x[::97] = np.nan
    c = rng.integers(0, 256, nmax + 16, dtype=np.uint8)
    dx, dc_in = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    codes = torch.empty(nmax + 48, dtype=torch.uint8, device="cuda")
    out = torch.empty(nmax + 48, dtype=torch.float32, device="cuda")
    want_e, want_d = ref_e(x), ref_d(c)
    for ox in range(16):
        for oc in range(16):
            for n in COUNTS:
                codes.fill_(0xA5)
                out.fill_(-7.0)
                torch.cuda.synchronize()
                q.quantize_device(dx.data_ptr() + 4 * ox, n, codes.data_ptr() + oc)
                q.dequantize_device(dc_in.data_ptr() + oc, n, out.data_ptr() + 4 * ox)
                _lib.synchronize()
                got_c, got_o = codes.cpu().numpy(), out.cpu().numpy()
                assert np.array_equal(got_c[oc:oc + n], want_e[ox:ox + n]), (ox, oc, n)
                assert (got_c[:oc] == 0xA5).all() and (got_c[oc + n:] == 0xA5).all(), (ox, oc, n)
                assert same_bits(got_o[ox:ox + n], want_d[oc:oc + n]), (ox, oc, n)
                assert (got_o[:ox] == -7.0).all() and (got_o[ox + n:] == -7.0).all(), (ox, oc, n)


def _check_chunked(x2d, got, ref):
    for r0 in range(0, x2d.shape[0], 65536):
        assert np.array_equal(got[r0:r0 + 65536], ref(x2d[r0:r0 + 65536])), r0


def test_full_size_1m_x_384_host_and_device():
    """1M x 384: the host form through the transfer lanes, the device form in one launch"""
    import torch

    import vq_amd
    from vq_amd import _lib

    n, d = 1_000_000, 384
    x = _lib.synth_uniform_host(n, d, seed=66)
    x = (x * F(2.2) - F(1.1)).astype(F)
    sq, bq = vq_amd.ScalarQuantizer(-1.0, 1.0, 256), vq_amd.BinaryQuantizer(0.0)
    lanes0 = _lib.xfer_lane_calls()
    codes = sq.quantize_batch(x)
    assert codes.shape == (n, d) and codes.dtype == np.uint8
    assert _lib.xfer_lane_calls() > lanes0
    _check_chunked(x, codes, lambda a: R.sq_encode(-1.0, 1.0, 256, a))
    out = np.empty((n, d), F)
    assert sq.dequantize_batch(codes, out=out) is out
    for r0 in range(0, n, 65536):
        assert same_bits(out[r0:r0 + 65536], R.sq_decode(-1.0, 1.0, 256, codes[r0:r0 + 65536]))
    dx = torch.from_numpy(x).cuda()
    dc = torch.empty((n, d), dtype=torch.uint8, device="cuda")
    do = torch.empty((n, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sq.quantize_device(dx.data_ptr(), n * d, dc.data_ptr())
    sq.dequantize_device(dc.data_ptr(), n * d, do.data_ptr())
    _lib.synchronize()
    assert np.array_equal(dc.cpu().numpy(), codes)
    assert same_bits(do.cpu().numpy(), out)
    bq.quantize_device(dx.data_ptr(), n * d, dc.data_ptr())
    _lib.synchronize()
    bcodes = dc.cpu().numpy()
    _check_chunked(x, bcodes, lambda a: R.bq_encode(0.0, 0, 1, a))
    assert np.array_equal(bq.quantize_batch(x), bcodes)


def test_per_vector_calls_and_batch_shapes():
    import vq_amd

    rng = np.random.default_rng(9)
    sq, bq = vq_amd.ScalarQuantizer(-1.0, 1.0), vq_amd.BinaryQuantizer(0.1, 2, 5)
    for _ in range(20):
        v = (rng.standard_normal(384) * 0.6).astype(F)
        c = sq.quantize(v)
        assert c.dtype == np.uint8 and c.shape == (384,)
        assert np.array_equal(c, R.sq_encode(-1.0, 1.0, 256, v))
        assert same_bits(sq.dequantize(c), R.sq_decode(-1.0, 1.0, 256, c))
        b = bq.quantize(v)
        assert np.array_equal(b, R.bq_encode(0.1, 2, 5, v))
        assert same_bits(bq.dequantize(b), R.bq_decode(0.1, 2, 5, b))
    X = (rng.standard_normal((3, 5, 7)) * 0.6).astype(F)
    assert np.array_equal(sq.quantize_batch(X), R.sq_encode(-1.0, 1.0, 256, X))
    out = np.empty((3, 5, 7), np.uint8)
    assert bq.quantize_batch(X, out=out) is out and np.array_equal(out, R.bq_encode(0.1, 2, 5, X))
    assert sq.quantize(np.empty(0, F)).shape == (0,) and sq.dequantize(np.empty(0, np.uint8)).shape == (0,)


def test_known_answers_fixture():
    import vq_amd

    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "sqbq_kat.json")))["cases"]
    for case in kat:
        kind, p = case["kind"], case["params"]
        x = np.array([F(s) for s in case["input"]], F)
        sq_like = kind.startswith("sq") or case.get("quantizer") == "sq"
        q = (vq_amd.ScalarQuantizer(F(p[0]), F(p[1]), p[2]) if sq_like else vq_amd.BinaryQuantizer(F(p[0]), p[1], p[2]))
        codes = q.quantize(x)
        assert codes.shape == x.shape, case["source"]
        if kind in ("bq_encode", "sq_encode"):
            assert codes.tolist() == case["expect"], case["source"]
        elif kind == "sq_roundtrip_bound":
            rec = q.dequantize(codes)
            clamped = np.clip(x, F(q.min), F(q.max))
            assert (np.abs(rec - clamped) <= F(q.step) / F(2) + F(1e-6)).all(), case["source"]
        elif kind == "bq_decode_in":
            assert set(q.dequantize(codes).tolist()) <= {float(F(v)) for v in case["values"]}, case["source"]


@pytest.mark.parametrize("alg", ["sq", "bq"])
def test_evalcli(alg, capsys):
    from vq_amd import evalcli

    assert evalcli.main([alg, "--samples", "1000", "--dim", "32"]) == 0
    text = capsys.readouterr().out
    assert ("Scalar" if alg == "sq" else "Binary") + " Quantizer Evaluation" in text
    assert "Samples: 1000" in text and "Quantization time" in text and "Reconstruction error" in text
