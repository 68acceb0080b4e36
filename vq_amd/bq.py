"""``BinaryQuantizer`` -- host mirror of the reference's threshold quantizer.

Same constructor (``low=0, high=1`` defaults), getters, ``repr`` and error text as
pyvq.BinaryQuantizer (reference pyvq/src/bq.rs) / ``BinaryQuantizer::new`` (src/bq.rs); low / high
outside 0..255 raise ``OverflowError`` as pyo3's u8 extraction does.  ``quantize`` / ``dequantize`` run
on the MI355X through libvqhip (vqhip_bq_*, vq_amd/csrc/k_sqbq.hip).
"""
from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import _lib
from .sq import f32_arg, rust_f32


def u8_arg(v) -> int:
    i = operator.index(v)
    if not 0 <= i <= 255:
        raise OverflowError("out of range integral type conversion attempted")
    return i


class BinaryQuantizer:
    """x >= threshold -> high, else low (NaN -> low); a code >= high decodes to high, any other to low."""

    def __init__(self, threshold: float, low: int = 0, high: int = 1):
        t, lo, hi = f32_arg(threshold), u8_arg(low), u8_arg(high)
        _lib.param_check(_lib.load().vqhip_bq_check(t, lo, hi))
        self._threshold, self._low, self._high = t, lo, hi

    @property
    def _params(self):
        return (self._threshold, self._low, self._high)

    # -- reference surface ----------------------------------------------------------------
    def quantize(self, values) -> np.ndarray:
        """float32 (n,) -> uint8 (n,)"""
        v = np.asarray(values, dtype=np.float32)
        if v.ndim != 1:
            raise ValueError("expected a 1D array")
        return self.quantize_batch(v)

    def dequantize(self, codes) -> np.ndarray:
        """uint8 (n,) -> float32 (n,)"""
        c = np.asarray(codes, dtype=np.uint8)
        if c.ndim != 1:
            raise ValueError("expected a 1D array")
        return self.dequantize_batch(c)

    @property
    def threshold(self) -> float:
        return float(self._threshold)

    @property
    def low(self) -> int:
        return self._low

    @property
    def high(self) -> int:
        return self._high

    def __repr__(self) -> str:  # pyvq/src/bq.rs __repr__
        return f"BinaryQuantizer(threshold={rust_f32(self._threshold)}, low={self._low}, high={self._high})"

    # -- batch additions ---------------------------------------------------------------------
    def quantize_batch(self, X, out=None) -> np.ndarray:
        """float32 array of any shape -> uint8 codes of the same shape; out: a uint8 array of that shape to fill"""
        return _lib.elementwise("vqhip_bq_encode", self._params, X, np.float32, np.uint8, out)

    def dequantize_batch(self, codes, out=None) -> np.ndarray:
        """uint8 codes of any shape -> float32 of the same shape; out: a float32 array of that shape to fill"""
        return _lib.elementwise("vqhip_bq_decode", self._params, codes, np.uint8, np.float32, out)

    def quantize_device(self, dev_x: int, count: int, dev_codes: int):
        """device pointers (x 4-byte aligned, any count), asynchronous on the current stream"""
        _lib.check(_lib.load().vqhip_bq_encode_device(*self._params, C.c_void_p(dev_x), int(count), C.c_void_p(dev_codes)))

    def dequantize_device(self, dev_codes: int, count: int, dev_out: int):
        _lib.check(_lib.load().vqhip_bq_decode_device(*self._params, C.c_void_p(dev_codes), int(count), C.c_void_p(dev_out)))
