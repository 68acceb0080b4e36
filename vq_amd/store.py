"""Code-based storage of a product-quantized set.

The reference's `quantize` hands back the f16 reconstruction (2 bytes per dimension,
src/pq.rs:165-199); the same information is the m one-byte codes per vector plus the codebooks
(C2: 8 bytes instead of 256 per vector).  `PQIndex` keeps exactly that and reproduces the
reference outputs from it: `reconstruct_f16()` == `quantize` of the encoded rows, bit for bit.

File layout (little endian), stable and trivially readable from C / Rust:

    0   8   magic  b"VQPQIDX1"
    8   4   u32    metric (0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine)
    12  4   u32    dim
    16  4   u32    m
    20  4   u32    k
    24  8   u64    n
    32  ..  f32    codebooks [m][k][dim/m]
    ..  ..  u8     codes     [n][m]        (k <= 256)
            u16    codes     [n][m]        (256 < k <= 65536, little endian; the library's code width)
"""
from __future__ import annotations

import struct

import numpy as np

from .distance import METRIC_NAMES, Distance

MAGIC = b"VQPQIDX1"
_HEADER = struct.Struct("<8sIIIIQ")


def _code_dtype(k: int):
    return np.dtype(np.uint8) if k <= 256 else np.dtype("<u2")


def _checked(codebooks, codes):
    """(codebooks f32 (m, k, sub_dim), codes (n, m) in the library's code width) after the checks of a store"""
    cb = np.ascontiguousarray(codebooks, dtype=np.float32)
    if cb.ndim != 3:
        raise ValueError("codebooks must have shape (m, k, sub_dim)")
    if cb.shape[1] > 65536:
        raise ValueError("codes are at most two bytes: k <= 65536")
    codes = np.asarray(codes)
    if codes.ndim != 2 or codes.shape[1] != cb.shape[0]:
        raise ValueError(f"codes must have shape (n, {cb.shape[0]})")
    if codes.size and (int(codes.min()) < 0 or int(codes.max()) >= cb.shape[1]):
        raise ValueError("code out of range for the codebooks")
    return cb, np.ascontiguousarray(codes, dtype=_code_dtype(cb.shape[1]))


class PQIndex:
    """codebooks + codes + distance.  `search` keeps an encoder with the codes on the device; reassigning `codes`,
    `codebooks` or `distance` drops it, so the next search answers for the new store.  Changing the arrays IN PLACE is
    not seen: reassign them after such a change."""

    def __init__(self, codebooks: np.ndarray, codes: np.ndarray, distance: Distance | None = None):
        self._codebooks, self._codes = _checked(codebooks, codes)
        self._distance = distance if distance is not None else Distance.euclidean()

    # -- the store (reassigning a part drops the device copy search keeps) ----------------------
    def _drop_encoder(self) -> None:
        enc = self.__dict__.pop("_enc", None)
        if enc is not None:
            enc.close()

    @property
    def codebooks(self) -> np.ndarray:
        return self._codebooks

    @codebooks.setter
    def codebooks(self, value) -> None:
        self._codebooks, self._codes = _checked(value, self._codes)
        self._drop_encoder()

    @property
    def codes(self) -> np.ndarray:
        return self._codes

    @codes.setter
    def codes(self, value) -> None:
        self._codebooks, self._codes = _checked(self._codebooks, value)
        self._drop_encoder()

    @property
    def distance(self) -> Distance:
        return self._distance

    @distance.setter
    def distance(self, value: Distance) -> None:
        self._distance = value
        self._drop_encoder()

    # -- shape ------------------------------------------------------------------------------
    @property
    def m(self) -> int:
        return self.codebooks.shape[0]

    @property
    def k(self) -> int:
        return self.codebooks.shape[1]

    @property
    def dim(self) -> int:
        return self.codebooks.shape[0] * self.codebooks.shape[2]

    def __len__(self) -> int:
        return self.codes.shape[0]

    @property
    def nbytes(self) -> int:
        return _HEADER.size + self.codebooks.nbytes + self.codes.nbytes

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def from_quantizer(cls, pq, X) -> "PQIndex":
        """encode X with a trained `ProductQuantizer` (device path) and keep the codes"""
        return cls(pq.codebooks, pq.encode(X), Distance(pq.distance_metric()))

    # -- reference-shaped outputs from the codes ----------------------------------------------
    def reconstruct(self, rows=None) -> np.ndarray:
        """(n, dim) float32: the selected centroids (host gather; the device path is pq.decode)"""
        codes = self.codes if rows is None else self.codes[rows]
        m, sd = self.m, self.codebooks.shape[2]
        out = np.empty((codes.shape[0], m * sd), np.float32)
        for s in range(m):
            out[:, s * sd:(s + 1) * sd] = self.codebooks[s][codes[:, s]]
        return out

    def reconstruct_f16(self, rows=None) -> np.ndarray:
        """what `ProductQuantizer::quantize` returned for these rows (f16, RNE; src/pq.rs:192-196)"""
        return self.reconstruct(rows).astype(np.float16)

    def search(self, queries, topk: int = 10, *, rerank=None, candidates: int | None = None, allowed=None):
        """top-k stored rows per query by asymmetric distance (device path; see ProductQuantizer.search, also for
        `rerank` / `candidates`: exact rerank of an ADC short list through a FlatIndex or a ScalarIndex over the same rows).
        Tables of m * k <= 38400 entries (one query's table in 150 KiB of LDS); larger ones raise FfiError
        (VQHIP_ERR_UNSUPPORTED).  Answers for the current codes, codebooks and distance (see the class).
        allowed: one row mask for the call, a bool array (n,) (True: the row may be returned) or its uint32 words
        (`pack_row_mask`) -- the nearest among the allowed rows only; a query with fewer than `topk` of them has the slots
        behind them padded with 0xFFFFFFFF / +inf (`topk` itself stays within 1 .. min(n, 1024)).  With `rerank`, the mask
        filters the first stage: its candidates are allowed rows."""
        from . import _lib
        from .errors import DimensionMismatch, InvalidParameter

        w = None
        if allowed is not None:
            from ._resident_common import _allowed

            w = _allowed(allowed, len(self))
        if rerank is not None:
            from .flat import adc_then_rerank

            q = np.ascontiguousarray(queries, dtype=np.float32)
            q = q[None, :] if q.ndim == 1 else q
            if w is not None:
                from ._ivf_common import filtered_adc_then_rerank

                return filtered_adc_then_rerank(lambda qq, c: self.search(qq, c, allowed=w), len(self), self.dim, q, topk, rerank,
                                                candidates)
            return adc_then_rerank(lambda qq, c: self.search(qq, c), len(self), self.dim, q, topk, rerank, candidates)

        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, q.shape[1])
        if not 1 <= topk <= min(len(self), 1024):
            raise InvalidParameter("topk", f"must be between 1 and min(n, 1024), got {topk}")
        if self.distance.metric in (_lib.COSINE, _lib.COSINE_UNCLAMPED):
            raise InvalidParameter("distance", "cosine distance is not a sum over subspaces: no ADC form")
        # the codes go to the device ONCE (checked against k there); later searches only send the queries, until a
        # reassignment of the store drops the encoder
        enc = self.__dict__.get("_enc")
        if enc is None:
            enc = _lib.PQEncoder(self.codebooks, self.distance.metric)
            enc.adc_set_codes(np.asarray(self.codes))
            self._enc = enc
        return enc.adc_search(None, q, int(topk), allowed=w)

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self.distance.metric, self.dim, self.m, self.k, len(self)))
            f.write(self.codebooks.tobytes())
            f.write(self.codes.tobytes())

    @classmethod
    def load(cls, path, mmap_codes: bool = False) -> "PQIndex":
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise ValueError("truncated index header")
            magic, metric, dim, m, k, n = _HEADER.unpack(head)
            if magic != MAGIC:
                raise ValueError("not a VQPQIDX1 file")
            if m == 0 or k == 0 or k > 65536 or dim == 0 or dim % m != 0 or metric >= len(METRIC_NAMES):
                raise ValueError("corrupt index header")
            sd = dim // m
            cb = np.frombuffer(f.read(m * k * sd * 4), dtype="<f4")
            if cb.size != m * k * sd:
                raise ValueError("truncated codebooks")
            off = f.tell()
            cdt = _code_dtype(k)
            if mmap_codes:
                codes = np.memmap(path, dtype=cdt, mode="r", offset=off, shape=(n, m))
            else:
                raw = f.read(n * m * cdt.itemsize)
                if len(raw) != n * m * cdt.itemsize:
                    raise ValueError("truncated codes")
                codes = np.frombuffer(raw, dtype=cdt).reshape(n, m)
        # k_adc_scan indexes the per-query LDS tables by code: a corrupt file must not get that far
        for r0 in range(0, n, 1 << 22):
            if codes[r0:r0 + (1 << 22)].size and int(codes[r0:r0 + (1 << 22)].max()) >= k:
                raise ValueError(f"corrupt index: a code is outside [0, {k})")
        self = cls.__new__(cls)  # (the codes, maybe a memmap, were checked above: not through _checked's copy)
        self._codebooks = cb.reshape(m, k, sd).astype(np.float32)
        self._codes = codes
        self._distance = Distance(METRIC_NAMES[metric])
        return self
