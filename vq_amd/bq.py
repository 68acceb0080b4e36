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

    def pack_batch(self, X, out=None) -> np.ndarray:
        """float32 (n, d) -> uint32 (n, ceil(d / 32)) on the device: bit t % 32 of word t // 32 is x[t] >= threshold
        (the layout of BinaryIndex, pad bits zero); out: a uint32 array of that shape to fill"""
        x = np.ascontiguousarray(X, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        n, d = x.shape
        if d == 0:
            raise ValueError("dimension must be at least 1")
        w = (d + 31) // 32
        if out is None:
            out = np.empty((n, w), np.uint32)
        elif out.dtype != np.uint32 or out.shape != (n, w) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint32 array of shape {(n, w)}")
        if n:
            _lib.check(_lib.load().vqhip_bq_pack(self._threshold, x.ctypes.data_as(C.POINTER(C.c_float)), n, d,
                                                 out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def unpack_batch(self, words, dim: int) -> np.ndarray:
        """uint32 (n, ceil(dim / 32)) packed bits -> uint8 codes (n, dim): high where the bit is set, else low (host)"""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        d = operator.index(dim)
        if w.ndim != 2 or d < 1 or w.shape[1] != (d + 31) // 32:
            raise ValueError(f"expected a 2D array (n, {(max(d, 1) + 31) // 32}) for dim {d}")
        bits = np.unpackbits(w.astype("<u4").view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :d]
        return np.where(bits.astype(bool), np.uint8(self._high), np.uint8(self._low))

    def quantize_device(self, dev_x: int, count: int, dev_codes: int):
        """device pointers (x 4-byte aligned, any count), asynchronous on the current stream"""
        _lib.check(_lib.load().vqhip_bq_encode_device(*self._params, C.c_void_p(dev_x), int(count), C.c_void_p(dev_codes)))

    def dequantize_device(self, dev_codes: int, count: int, dev_out: int):
        _lib.check(_lib.load().vqhip_bq_decode_device(*self._params, C.c_void_p(dev_codes), int(count), C.c_void_p(dev_out)))
