"""CPU-side checks of ScalarQuantizer / BinaryQuantizer (vq_amd/sq.py, vq_amd/bq.py, vqhip_sq_* / vqhip_bq_*): the
reference's validation order and texts (Python, the C ABI), repr and getters as pyvq prints them, the threshold table
the encode kernel corrects its estimate with -- proved against the numpy restatement of src/sq.rs -- and no CPU
fallback."""
import ctypes

import numpy as np
import pytest

import ref_sqbq as R

F = np.float32
NAN, INF = float("nan"), float("inf")

SQ_BAD = [  # (args, parameter, reason): src/sq.rs ScalarQuantizer::new checks, in order
    ((NAN, 1.0, 256), "min", "must be finite (not NaN or infinite)"),
    ((NAN, NAN, 0), "min", "must be finite (not NaN or infinite)"),
    ((-INF, 1.0, 256), "min", "must be finite (not NaN or infinite)"),
    ((-1.0, NAN, 256), "max", "must be finite (not NaN or infinite)"),
    ((-1.0, INF, 0), "max", "must be finite (not NaN or infinite)"),
    ((1.0, -1.0, 5), "max", "must be greater than min"),
    ((1.0, 1.0, 0), "max", "must be greater than min"),
    ((-1.0, 1.0, 1), "levels", "must be at least 2"),
    ((-1.0, 1.0, 0), "levels", "must be at least 2"),
    ((0.0, 1.0, 257), "levels", "must be no more than 256 to fit in u8"),
    ((0.0, 1.0, 300), "levels", "must be no more than 256 to fit in u8"),
    ((0.0, 1e39, 256), "max", "must be finite (not NaN or infinite)"),  # rounds to +inf as an f32
]
BQ_BAD = [
    ((NAN, 0, 1), "threshold", "must be finite (not NaN or infinite)"),
    ((NAN, 1, 0), "threshold", "must be finite (not NaN or infinite)"),
    ((INF, 0, 1), "threshold", "must be finite (not NaN or infinite)"),
    ((0.0, 5, 5), "low/high", "low must be less than high"),
    ((0.0, 6, 5), "low/high", "low must be less than high"),
    ((0.0, 1, 0), "low/high", "low must be less than high"),
]


@pytest.fixture(scope="module")
def lib():
    from vq_amd import _lib

    return _lib


@pytest.mark.parametrize("args,parameter,reason", SQ_BAD)
def test_sq_validation_python_and_cabi(lib, args, parameter, reason):
    import vq_amd

    with pytest.raises(vq_amd.InvalidParameter) as e:
        vq_amd.ScalarQuantizer(*args)
    assert (e.value.parameter, e.value.reason) == (parameter, reason)
    assert str(e.value) == f"Invalid parameter '{parameter}': {reason}"
    assert isinstance(e.value, ValueError)  # pyvq raises ValueError(e.to_string())
    step = ctypes.c_float(0)
    from vq_amd.sq import f32_arg

    assert lib.load().vqhip_sq_check(f32_arg(args[0]), f32_arg(args[1]), args[2], ctypes.byref(step)) == lib.ERR_INVALID_INPUT
    assert lib.last_error() == str(e.value)


@pytest.mark.parametrize("args,parameter,reason", BQ_BAD)
def test_bq_validation_python_and_cabi(lib, args, parameter, reason):
    import vq_amd

    with pytest.raises(vq_amd.InvalidParameter) as e:
        vq_amd.BinaryQuantizer(*args)
    assert (e.value.parameter, e.value.reason) == (parameter, reason)
    assert lib.load().vqhip_bq_check(*args) == lib.ERR_INVALID_INPUT
    assert lib.last_error() == str(e.value)


def test_argument_types_like_pyo3():
    import vq_amd

    for bad in (-1, 256, 1000):
        with pytest.raises(OverflowError):
            vq_amd.BinaryQuantizer(0.0, bad, 1) if bad < 0 else vq_amd.BinaryQuantizer(0.0, 0, bad)
    with pytest.raises(OverflowError):
        vq_amd.ScalarQuantizer(0.0, 1.0, -1)
    with pytest.raises(TypeError):
        vq_amd.ScalarQuantizer(0.0, 1.0, 2.5)
    with pytest.raises(vq_amd.InvalidParameter):  # beyond u32: still "no more than 256"
        vq_amd.ScalarQuantizer(0.0, 1.0, 1 << 40)


def test_repr_and_getters():
    import vq_amd

    sq = vq_amd.ScalarQuantizer(-1.0, 1.0)
    assert repr(sq) == "ScalarQuantizer(min=-1, max=1, levels=256)"
    assert (sq.min, sq.max, sq.levels) == (-1.0, 1.0, 256)
    assert sq.step == float(F(2.0) / F(255.0))
    assert repr(vq_amd.ScalarQuantizer(0.5, 0.75, 3)) == "ScalarQuantizer(min=0.5, max=0.75, levels=3)"
    assert repr(vq_amd.ScalarQuantizer(1e-7, 0.1, 2)) == "ScalarQuantizer(min=0.0000001, max=0.1, levels=2)"
    assert repr(vq_amd.ScalarQuantizer(-3e38, 3e38, 256)) == (
        "ScalarQuantizer(min=-300000000000000000000000000000000000000, max=300000000000000000000000000000000000000, levels=256)")
    assert vq_amd.ScalarQuantizer(0.1, 0.2, 2).min == float(F(0.1))  # the f32 value, as pyvq returns it
    assert vq_amd.ScalarQuantizer(-3e38, 3e38, 256).step == INF
    assert vq_amd.ScalarQuantizer(0.0, 1e-45, 3).step == 0.0
    bq = vq_amd.BinaryQuantizer(0.5, 10, 20)  # src/bq.rs test_getters
    assert (bq.threshold, bq.low, bq.high) == (0.5, 10, 20)
    assert repr(bq) == "BinaryQuantizer(threshold=0.5, low=10, high=20)"
    assert repr(vq_amd.BinaryQuantizer(0.0)) == "BinaryQuantizer(threshold=0, low=0, high=1)"
    assert repr(vq_amd.BinaryQuantizer(-0.0)) == "BinaryQuantizer(threshold=-0, low=0, high=1)"
    assert repr(vq_amd.BinaryQuantizer(-2.5, 0, 255)) == "BinaryQuantizer(threshold=-2.5, low=0, high=255)"


def test_step_and_check_agree_with_restatement(lib):
    for cfg in R.SQ_CONFIGS:
        step = ctypes.c_float(-1)
        assert lib.load().vqhip_sq_check(*cfg, ctypes.byref(step)) == lib.OK
        assert F(step.value).view(np.uint32) == R.sq_step(*cfg).view(np.uint32), cfg
    assert lib.load().vqhip_sq_check(0.0, 1.0, 256, None) == lib.OK
    assert lib.load().vqhip_bq_check(0.0, 0, 255) == lib.OK
    assert lib.load().vqhip_bq_check(0.0, 0, 256) == lib.ERR_INVALID_INPUT  # u8 in the reference


@pytest.mark.parametrize("cfg", R.SQ_CONFIGS, ids=[f"{a:g},{b:g},{c}" for a, b, c in R.SQ_CONFIGS])
def test_threshold_table_is_exact(cfg):
    """b[i] is the smallest f32 whose code is >= i: code(b[i]) >= i and code(prevfloat(b[i])) < i -- with the map's
    monotonicity that is the whole map"""
    import vq_amd

    sq = vq_amd.ScalarQuantizer(*cfg)
    b = sq.thresholds()
    assert b.shape == (cfg[2],) and b[0] == -INF
    i = np.arange(1, cfg[2])
    have = ~np.isnan(b[1:])
    top_code = int(R.sq_encode(*cfg, np.array([INF], F))[0])
    assert (i[~have] > top_code).all()  # "no input reaches i" only when +inf does not
    bi, ii = b[1:][have], i[have]
    assert (R.sq_encode(*cfg, bi).astype(int) >= ii).all()
    assert (R.sq_encode(*cfg, R.nextafter32(bi, -np.inf)).astype(int) < ii).all()
    assert (np.diff(bi) >= 0).all()
    # and a dense spot check of monotonicity itself around every threshold
    around = np.sort(np.concatenate([bi, R.nextafter32(bi, np.inf), R.nextafter32(bi, -np.inf)]))
    assert (np.diff(R.sq_encode(*cfg, around).astype(int)) >= 0).all()


def test_restatement_known_answers():
    """the restatement itself against the reference's in-test answers and the degenerate steps of the spec"""
    assert R.sq_encode(0.0, 1.0, 11, [0.0, 0.5, 1.0]).tolist() == [0, 5, 10]  # src/sq.rs doc example
    assert R.bq_encode(0.0, 0, 1, [-1.0, 0.0, 1.0, -0.5, 0.5]).tolist() == [0, 1, 1, 0, 1]  # src/bq.rs test_basic
    assert R.round_half_away(np.array([0.49999997, 0.5, -0.5, 2.5, -2.5, INF, NAN], F))[:6].tolist() == [0, 1, -1, 3, -3, INF]
    assert R.sq_encode(-3e38, 3e38, 256, [3e38, -3e38, 0.0, INF]).tolist() == [0, 0, 0, 0]
    assert R.sq_encode(0.0, 1e-45, 3, [0.0, 1e-45, NAN, -INF, INF]).tolist() == [0, 2, 0, 0, 2]
    assert R.sq_encode(-1.0, 1.0, 256, [NAN, INF, -INF]).tolist() == [0, 255, 0]


def _gpu_present():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="this check is about machines WITHOUT a GPU")
def test_encode_without_gpu_raises_ffi_error():
    import vq_amd

    sq, bq = vq_amd.ScalarQuantizer(-1.0, 1.0), vq_amd.BinaryQuantizer(0.0)
    for fn in (lambda: sq.quantize(np.zeros(4, F)), lambda: sq.dequantize(np.zeros(4, np.uint8)),
               lambda: bq.quantize_batch(np.zeros((2, 3), F)), lambda: bq.dequantize(np.zeros(4, np.uint8))):
        with pytest.raises(vq_amd.FfiError) as e:
            fn()
        assert "no CPU fallback" in str(e.value)
    # empty input is empty output, before any device is needed (src/bq.rs test_empty_input)
    assert sq.quantize(np.zeros(0, F)).shape == (0,) and bq.dequantize(np.zeros(0, np.uint8)).shape == (0,)
