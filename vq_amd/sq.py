"""``ScalarQuantizer`` -- host mirror of the reference's uniform scalar quantizer.

Same constructor (``levels=256`` default), getters, ``repr`` and error text as pyvq.ScalarQuantizer
(reference pyvq/src/sq.rs) / ``ScalarQuantizer::new`` (src/sq.rs).  ``quantize`` / ``dequantize`` run
on the MI355X through libvqhip (vqhip_sq_*, vq_amd/csrc/k_sqbq.hip) and give the reference's codes and
values bit for bit: NaN -> 0, +-inf -> the end codes, the degenerate steps (inf, 0) included.
"""
from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import _lib
from .errors import DimensionMismatch, InvalidParameter


def f32_arg(v) -> np.float32:
    """pyo3's f32 extraction: the Python float rounded to f32 (out of range -> +-inf)"""
    with np.errstate(over="ignore"):
        return np.float32(float(v))


def usize_arg(v) -> int:
    i = operator.index(v)
    if i < 0:
        raise OverflowError("can't convert negative int to unsigned")
    return i


def rust_f32(v) -> str:
    """Rust's `Display` of an f32: the shortest digits that round-trip, never an exponent"""
    return np.format_float_positional(np.float32(v), unique=True, trim="-")


class ScalarQuantizer:
    """Uniform scalar quantizer of [min, max] into `levels` codes (2..256)."""

    def __init__(self, min: float, max: float, levels: int = 256):
        mn, mx = f32_arg(min), f32_arg(max)
        lv = usize_arg(levels)
        step = C.c_float(0)
        # levels beyond u32 fail the same "no more than 256" check as any value above 256
        _lib.param_check(_lib.load().vqhip_sq_check(mn, mx, lv if lv <= 0xFFFFFFFF else 0xFFFFFFFF, C.byref(step)))
        self._min, self._max, self._levels, self._step = mn, mx, lv, np.float32(step.value)

    @property
    def _params(self):
        return (self._min, self._max, self._levels)

    # -- reference surface ----------------------------------------------------------------
    def quantize(self, values) -> np.ndarray:
        """float32 (n,) -> uint8 (n,)"""
        v = np.asarray(values, dtype=np.float32)
        if v.ndim != 1:
            raise ValueError("expected a 1D array")
        return self.quantize_batch(v)

    def dequantize(self, codes) -> np.ndarray:
        """uint8 (n,) -> float32 (n,): min + code * step for every code"""
        c = np.asarray(codes, dtype=np.uint8)
        if c.ndim != 1:
            raise ValueError("expected a 1D array")
        return self.dequantize_batch(c)

    @property
    def min(self) -> float:
        return float(self._min)

    @property
    def max(self) -> float:
        return float(self._max)

    @property
    def levels(self) -> int:
        return self._levels

    @property
    def step(self) -> float:
        return float(self._step)

    def __repr__(self) -> str:  # pyvq/src/sq.rs __repr__
        return f"ScalarQuantizer(min={rust_f32(self._min)}, max={rust_f32(self._max)}, levels={self._levels})"

    # -- batch additions ---------------------------------------------------------------------
    def quantize_batch(self, X, out=None) -> np.ndarray:
        """float32 array of any shape -> uint8 codes of the same shape; out: a uint8 array of that shape to fill"""
        return _lib.elementwise("vqhip_sq_encode", self._params, X, np.float32, np.uint8, out)

    def dequantize_batch(self, codes, out=None) -> np.ndarray:
        """uint8 codes of any shape -> float32 of the same shape; out: a float32 array of that shape to fill"""
        return _lib.elementwise("vqhip_sq_decode", self._params, codes, np.uint8, np.float32, out)

    def quantize_device(self, dev_x: int, count: int, dev_codes: int):
        """device pointers (x 4-byte aligned, any count), asynchronous on the current stream"""
        _lib.check(_lib.load().vqhip_sq_encode_device(*self._params, C.c_void_p(dev_x), int(count), C.c_void_p(dev_codes)))

    def dequantize_device(self, dev_codes: int, count: int, dev_out: int):
        _lib.check(_lib.load().vqhip_sq_decode_device(*self._params, C.c_void_p(dev_codes), int(count), C.c_void_p(dev_out)))

    # -- the 4-bit layout of Scalar4Index (include/vqhip.h, "4-bit scalar index"), on the host ----------------------
    @staticmethod
    def pack4_codes(codes) -> np.ndarray:
        """uint8 codes (n, d), each <= 15 -> uint32 words (n, ceil(d / 8)): dimension t of a row is bits 4 (t % 8) ..
        4 (t % 8) + 3 of its word t // 8, pad nibbles zero"""
        c = codes if isinstance(codes, np.ndarray) else np.asarray(codes)
        if c.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {c.dtype}")
        if c.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        if c.size and int(c.max()) > 15:
            raise InvalidParameter("codes", f"a 4-bit code is at most 15, got {int(c.max())}")
        n, d = c.shape
        w = (d + 7) // 8
        p = np.zeros((n, w * 8), np.uint32)
        p[:, :d] = c
        p = p.reshape(n, w, 8)
        out = np.zeros((n, w), np.uint32)
        for j in range(8):
            out |= p[:, :, j] << np.uint32(4 * j)
        return out

    @staticmethod
    def unpack4_batch(words, dim: int) -> np.ndarray:
        """uint32 words (n, ceil(dim / 8)) in ``pack4_codes``' layout -> uint8 codes (n, dim); the pad nibbles are not
        read"""
        a = words if isinstance(words, np.ndarray) else np.asarray(words)
        if a.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {a.dtype}")
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, words)")
        d = usize_arg(dim)
        if d < 1:
            raise InvalidParameter("dim", "must be at least 1")
        if a.shape[1] != (d + 7) // 8:
            raise DimensionMismatch((d + 7) // 8, a.shape[1])
        shifts = (np.arange(8, dtype=np.uint32) * np.uint32(4))[None, None, :]
        c = (a[:, :, None] >> shifts) & np.uint32(15)
        return np.ascontiguousarray(c.reshape(a.shape[0], -1)[:, :d].astype(np.uint8))

    def thresholds(self) -> np.ndarray:
        """float32 (levels,): [0] = -inf, [i] = the smallest input whose code is >= i (NaN if none) -- the table the
        encode kernel corrects its estimate with"""
        b = np.empty(self._levels, np.float32)
        _lib.check(_lib.load().vqhip_sq_thresholds(*self._params, _lib.ptr(b, _lib._f32p)))
        return b
