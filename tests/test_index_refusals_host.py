"""Refused calls of the ten search indexes, and refused index files: which exception, with which words.  Every case is a
wrong call that the Python layer refuses before the library or a device is reached -- constructors, ``from_packed``,
every ``add*`` form (wrong number of dimensions, width, dtype, count, list id, pad bit or nibble, code above the limit,
and pairs of these at once: which of two faults is reported is behaviour), ``nq`` of every device-form call -- or a
corrupt file of one of the nine formats (short header, wrong magic, each header field out of range, each block short of
one byte, a trailing byte, a list id equal to nlist, a pad bit, a pad nibble, a code equal to k).

The expected ``(exception class name, str(exception))`` of every case is a recorded result,
tests/golden/index_refusals.json, written by ``PYTHONPATH=. python tests/test_index_refusals_host.py`` at commit 1716bef
("Time encode stages from the kernels' dispatches; no exit marker"), the parent of the change that gave the indexes one
host layer for add checks, payloads and files; the test only compares.  Not expressed: an add refused for want of room
below 2^32 rows in an inverted file, which needs that many rows first.  No GPU."""
import json
import os
import struct
import tempfile

import numpy as np
import pytest

from vq_amd import (AsymmetricBinaryIndex, BinaryIndex, BinaryQuantizer, Distance, FlatIndex, IVFBinaryIndex, IVFFlatIndex,
                    IVFPQIndex, IVFScalar4Index, IVFScalarIndex, Scalar4Index, ScalarIndex, ScalarQuantizer)
from vq_amd.binary import pack_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_refusals.json")
F = np.float32
NLIST, N = 3, 6
DIM = 11  # two 4-bit words a row, the second with five pad nibbles; one 1-bit word with 21 pad bits
M, K = 1, 16  # IVFPQIndex: DIM is prime, so one subspace
SQ, SQ4, BQ = ScalarQuantizer(-3.0, 5.0, 17), ScalarQuantizer(-3.0, 5.0, 9), BinaryQuantizer(0.25, 3, 200)
BAD_NQ = {"negative": -1, "2^32": 1 << 32, "float": 1.5}


def _data():
    rng = np.random.default_rng(20261021)
    d = dict(coarse=rng.standard_normal((NLIST, DIM)).astype(F), lists=rng.integers(0, NLIST, N).astype(np.uint32),
             rows=rng.standard_normal((N, DIM)).astype(F), cb=rng.standard_normal((M, K, DIM // M)).astype(F),
             pq=rng.integers(0, K, (N, M)).astype(np.uint8), u8=rng.integers(0, 256, (N, DIM)).astype(np.uint8),
             c4=rng.integers(0, 16, (N, DIM)).astype(np.uint8), bits=rng.integers(0, 2, (N, DIM)).astype(bool))
    d["w4"] = ScalarQuantizer.pack4_codes(d["c4"])
    d["w1"] = pack_bits(d["bits"])
    return d


D = _data()


def _pad(words):
    """the words with the highest bit of the first row's last word set: a pad bit, a pad nibble"""
    w = words.copy()
    w[0, -1] |= np.uint32(1 << 31)
    return w


def _ivf(kind):
    """a valid index of N rows, host only"""
    if kind == "ivfpq":
        ix = IVFPQIndex(D["coarse"], D["cb"], Distance.squared_euclidean())
        ix.add_codes(D["lists"], D["pq"])
    elif kind == "ivfpq_residual":
        ix = IVFPQIndex(D["coarse"], D["cb"], Distance.manhattan(), residual=True)
        ix.add_codes(D["lists"], D["pq"])
    elif kind == "ivfflat":
        ix = IVFFlatIndex(D["coarse"], Distance.cosine())
        ix.add_rows(D["lists"], D["rows"])
    elif kind == "ivfflat_f16":
        ix = IVFFlatIndex(D["coarse"], Distance.euclidean(), np.float16)
        ix.add_rows(D["lists"], D["rows"])
    elif kind == "ivfsq":
        ix = IVFScalarIndex(D["coarse"], SQ, Distance.manhattan())
        ix.add_codes(D["lists"], D["u8"])
    elif kind == "ivfsq4":
        ix = IVFScalar4Index(D["coarse"], SQ4, Distance.cosine())
        ix.add_codes(D["lists"], D["c4"])
    else:
        ix = IVFBinaryIndex(D["coarse"], BQ, Distance.squared_euclidean(), Distance.cosine())
        ix.add_packed(D["lists"], D["w1"])
    return ix


def _resident(kind):
    if kind == "flat":
        return FlatIndex(D["rows"], Distance.cosine())
    if kind == "sq":
        return ScalarIndex.from_codes(D["u8"], SQ, Distance.manhattan())
    if kind == "sq4":
        return Scalar4Index.from_packed(D["w4"], DIM, SQ4, Distance.cosine())
    if kind == "bin":
        return BinaryIndex.from_packed(D["w1"], DIM, BQ, Distance.euclidean())
    return AsymmetricBinaryIndex.from_packed(D["w1"], DIM, BQ, Distance.cosine())


# ---- wrong calls -------------------------------------------------------------------------------------------------------

def _array_faults(good, other_dtype, width_name="width"):
    """wrong forms of the 2-D array `good` that an add takes: (name, array)"""
    return [("1d", good[0]), ("3d", good[None]), (width_name, np.concatenate([good, good[:, :1]], axis=1)),
            ("narrow", good[:, :-1]), ("dtype", good.astype(other_dtype)), ("count", good[:-1]),
            ("1d_dtype", good[0].astype(other_dtype)), ("width_dtype", good[:, :-1].astype(other_dtype)),
            ("width_count", good[:-1, :-1]), ("dtype_count", good[:-1].astype(other_dtype))]


def _list_faults(lists):
    bad = lists.astype(np.int64)
    bad[2] = NLIST
    neg = lists.astype(np.int64)
    neg[0] = -1
    return [("lists_2d", lists[None]), ("lists_0d", np.uint32(1)), ("list_out_of_range", bad), ("list_negative", neg),
            ("lists_float", lists.astype(np.float64))]


def _ivf_add_cases(out, kind, method, good, other_dtype, value_faults=()):
    """wrong calls of ``method(list_ids, array)`` of the inverted file `kind`; value_faults: (name, array) with the right
    shape and dtype and a refused value"""
    lists = D["lists"]
    bad = lists.astype(np.int64)
    bad[2] = NLIST

    def call(l, a):
        return lambda: getattr(_ivf(kind), method)(l, a)

    for name, a in _array_faults(good, other_dtype):
        out[f"{kind}.{method}:{name}"] = call(lists, a)
        out[f"{kind}.{method}:{name}+list_out_of_range"] = call(bad, a)
        out[f"{kind}.{method}:{name}+lists_2d"] = call(lists[None], a)
    for name, l in _list_faults(lists):
        out[f"{kind}.{method}:{name}"] = call(l, good)
    for name, a in value_faults:
        out[f"{kind}.{method}:{name}"] = call(lists, a)
        out[f"{kind}.{method}:{name}+list_out_of_range"] = call(bad, a)
        out[f"{kind}.{method}:{name}+count"] = call(lists, a[:-1])
        out[f"{kind}.{method}:{name}+width"] = call(lists, a[:, 1:])
        out[f"{kind}.{method}:{name}+dtype"] = call(lists, a.astype(np.int64))


def _resident_add_cases(out, kind, method, good, other_dtype, value_faults=()):
    """wrong calls of ``method(array)`` of the resident index `kind`, each refused before the index goes to the device"""
    def call(a):
        return lambda: getattr(_resident(kind), method)(a)

    for name, a in _array_faults(good, other_dtype):
        if "count" not in name:
            out[f"{kind}.{method}:{name}"] = call(a)
    for name, a in value_faults:
        out[f"{kind}.{method}:{name}"] = call(a)
        out[f"{kind}.{method}:{name}+width"] = call(a[:, 1:])
        out[f"{kind}.{method}:{name}+dtype"] = call(a.astype(np.int64))
        out[f"{kind}.{method}:{name}+1d"] = call(a[0])


def _device_n_cases(out, kind, make, method):
    """the count of a device-form add: refused before the device"""
    for name, n in (("negative", -1), ("float", 1.5), ("2^32", 1 << 32)):
        out[f"{kind}.{method}:n_{name}"] = (lambda n=n: getattr(make(kind), method)(0, n))


def _nq_cases(out, kind, make, forms):
    """forms: (name, call(ix, nq)) of every device-form call of the index"""
    for form, call in forms:
        for name, nq in BAD_NQ.items():
            out[f"{kind}.{form}:nq_{name}"] = (lambda call=call, nq=nq: call(make(kind), nq))


def _constructor_cases(out):
    c, cb = D["coarse"], D["cb"]
    big = np.zeros((65537, 1), F)
    cos = Distance.cosine()
    for name, f in {
        # the inverted files
        "ivfpq:coarse_1d": lambda: IVFPQIndex(c[0], cb), "ivfpq:codebooks_2d": lambda: IVFPQIndex(c, cb[0]),
        "ivfpq:distance_type": lambda: IVFPQIndex(c, cb, "euclidean"), "ivfpq:cosine": lambda: IVFPQIndex(c, cb, cos),
        "ivfpq:residual_type": lambda: IVFPQIndex(c, cb, residual=1), "ivfpq:nlist_0": lambda: IVFPQIndex(c[:0], cb),
        "ivfpq:nlist_big": lambda: IVFPQIndex(big, np.zeros((1, 2, 1), F)),
        "ivfpq:m_0": lambda: IVFPQIndex(c, cb[:0]), "ivfpq:k_big": lambda: IVFPQIndex(c, np.zeros((1, 65537, DIM), F)),
        "ivfpq:table": lambda: IVFPQIndex(np.zeros((2, 4), F), np.zeros((4, 9601, 1), F)),
        "ivfpq:dim": lambda: IVFPQIndex(c, cb[:, :, :-1]),
        "ivfpq:coarse_1d+cosine": lambda: IVFPQIndex(c[0], cb, cos),
        "ivfflat:coarse_1d": lambda: IVFFlatIndex(c[0]), "ivfflat:coarse_3d": lambda: IVFFlatIndex(c[None]),
        "ivfflat:nlist_0": lambda: IVFFlatIndex(c[:0]), "ivfflat:nlist_big": lambda: IVFFlatIndex(big),
        "ivfflat:dim_0": lambda: IVFFlatIndex(c[:, :0]), "ivfflat:distance_type": lambda: IVFFlatIndex(c, "cosine"),
        "ivfflat:dtype": lambda: IVFFlatIndex(c, None, np.float64), "ivfflat:dtype_name": lambda: IVFFlatIndex(c, None, "rows"),
        "ivfflat:coarse_1d+dtype": lambda: IVFFlatIndex(c[0], None, np.int8),
        "ivfflat:distance_type+coarse_1d": lambda: IVFFlatIndex(c[0], 3),
        "ivfsq:quantizer_type": lambda: IVFScalarIndex(c, BQ), "ivfsq:quantizer_none": lambda: IVFScalarIndex(c, None),
        "ivfsq:distance_type": lambda: IVFScalarIndex(c, SQ, "cosine"), "ivfsq:coarse_1d": lambda: IVFScalarIndex(c[0], SQ),
        "ivfsq:nlist_0": lambda: IVFScalarIndex(c[:0], SQ), "ivfsq:dim_0": lambda: IVFScalarIndex(c[:, :0], SQ),
        "ivfsq:quantizer_type+coarse_1d": lambda: IVFScalarIndex(c[0], 7),
        "ivfsq:train_quantizer_type": lambda: IVFScalarIndex.train(D["rows"], 2, BQ),
        "ivfsq4:quantizer_type": lambda: IVFScalar4Index(c, BQ), "ivfsq4:levels": lambda: IVFScalar4Index(c, SQ),
        "ivfsq4:distance_type": lambda: IVFScalar4Index(c, SQ4, "cosine"), "ivfsq4:coarse_1d": lambda: IVFScalar4Index(c[0], SQ4),
        "ivfsq4:nlist_0": lambda: IVFScalar4Index(c[:0], SQ4), "ivfsq4:dim_0": lambda: IVFScalar4Index(c[:, :0], SQ4),
        "ivfsq4:levels+coarse_1d": lambda: IVFScalar4Index(c[0], SQ),
        "ivfsq4:train_levels": lambda: IVFScalar4Index.train(D["rows"], 2, SQ),
        "ivfbin:quantizer_type": lambda: IVFBinaryIndex(c, SQ), "ivfbin:distance_type": lambda: IVFBinaryIndex(c, BQ, "manhattan"),
        "ivfbin:cosine": lambda: IVFBinaryIndex(c, BQ, cos), "ivfbin:coarse_distance_type": lambda: IVFBinaryIndex(c, BQ, None, 2),
        "ivfbin:coarse_1d": lambda: IVFBinaryIndex(c[0]), "ivfbin:nlist_0": lambda: IVFBinaryIndex(c[:0]),
        "ivfbin:dim_0": lambda: IVFBinaryIndex(c[:, :0]), "ivfbin:dim_big": lambda: IVFBinaryIndex(np.zeros((2, 8193), F)),
        "ivfbin:cosine+coarse_1d": lambda: IVFBinaryIndex(c[0], BQ, cos),
        "ivfbin:coarse_distance_type+quantizer_type": lambda: IVFBinaryIndex(c, SQ, None, 2),
        "ivfbin:train_quantizer_type": lambda: IVFBinaryIndex.train(D["rows"], 2, SQ),
        "ivfbin:train_coarse_distance_type": lambda: IVFBinaryIndex.train(D["rows"], 2, BQ, coarse_distance="cosine"),
        # the resident indexes
        "flat:dtype": lambda: FlatIndex(D["rows"].astype(np.float64)), "flat:1d": lambda: FlatIndex(D["rows"][0]),
        "flat:empty": lambda: FlatIndex(D["rows"][:0]), "flat:dim_0": lambda: FlatIndex(D["rows"][:, :0]),
        "flat:distance_type": lambda: FlatIndex(D["rows"], "cosine"), "flat:distance_type+dtype": lambda: FlatIndex(D["u8"], 1),
        "sq:dtype": lambda: ScalarIndex(D["u8"], SQ), "sq:1d": lambda: ScalarIndex(D["rows"][0], SQ),
        "sq:empty": lambda: ScalarIndex(D["rows"][:0], SQ), "sq:dim_0": lambda: ScalarIndex(D["rows"][:, :0], SQ),
        "sq:quantizer_type": lambda: ScalarIndex(D["rows"], BQ), "sq:distance_type": lambda: ScalarIndex(D["rows"], SQ, "cosine"),
        "sq:from_codes_dtype": lambda: ScalarIndex.from_codes(D["rows"], SQ),
        "sq:from_codes_1d": lambda: ScalarIndex.from_codes(D["u8"][0], SQ),
        "sq:from_codes_dtype+quantizer_type": lambda: ScalarIndex.from_codes(D["rows"], BQ),
        "sq:from_codes_1d+quantizer_type": lambda: ScalarIndex.from_codes(D["u8"][0], BQ),
        "sq4:dtype": lambda: Scalar4Index(D["u8"], SQ4), "sq4:1d": lambda: Scalar4Index(D["rows"][0], SQ4),
        "sq4:empty": lambda: Scalar4Index(D["rows"][:0], SQ4), "sq4:levels": lambda: Scalar4Index(D["rows"], SQ),
        "sq4:quantizer_type": lambda: Scalar4Index(D["rows"], BQ), "sq4:distance_type": lambda: Scalar4Index(D["rows"], SQ4, 0),
        "sq4:from_codes_dtype": lambda: Scalar4Index.from_codes(D["rows"], SQ4),
        "sq4:from_codes_above_15": lambda: Scalar4Index.from_codes(D["u8"], SQ4),
        "sq4:from_codes_above_15+levels": lambda: Scalar4Index.from_codes(D["u8"], SQ),
        "sq4:from_codes_above_15+1d": lambda: Scalar4Index.from_codes(D["u8"][0], SQ4),
        "sq4:from_codes_levels": lambda: Scalar4Index.from_codes(D["c4"], SQ),
        "bin:dtype": lambda: BinaryIndex(D["u8"]), "bin:1d": lambda: BinaryIndex(D["rows"][0]),
        "bin:empty": lambda: BinaryIndex(D["rows"][:0]), "bin:dim_0": lambda: BinaryIndex(D["rows"][:, :0]),
        "bin:dim_big": lambda: BinaryIndex(np.zeros((1, 8193), F)), "bin:quantizer_type": lambda: BinaryIndex(D["rows"], SQ),
        "bin:distance_type": lambda: BinaryIndex(D["rows"], BQ, "manhattan"), "bin:cosine": lambda: BinaryIndex(D["rows"], BQ, cos),
        "bin:cosine+quantizer_type": lambda: BinaryIndex(D["rows"], SQ, cos),
        "bin:from_codes_dtype": lambda: BinaryIndex.from_codes(D["rows"]),
        "bin:from_codes_1d": lambda: BinaryIndex.from_codes(D["u8"][0]),
        "bin:from_codes_cosine": lambda: BinaryIndex.from_codes(D["u8"], BQ, cos),
        "abin:dtype": lambda: AsymmetricBinaryIndex(D["u8"]), "abin:1d": lambda: AsymmetricBinaryIndex(D["rows"][0]),
        "abin:empty": lambda: AsymmetricBinaryIndex(D["rows"][:0]), "abin:dim_0": lambda: AsymmetricBinaryIndex(D["rows"][:, :0]),
        "abin:dim_big": lambda: AsymmetricBinaryIndex(np.zeros((1, 8193), F)),
        "abin:quantizer_type": lambda: AsymmetricBinaryIndex(D["rows"], SQ),
        "abin:distance_type": lambda: AsymmetricBinaryIndex(D["rows"], BQ, "cosine"),
        "abin:distance_type+quantizer_type": lambda: AsymmetricBinaryIndex(D["rows"], SQ, "cosine"),
        "abin:from_codes_dtype": lambda: AsymmetricBinaryIndex.from_codes(D["rows"]),
        "abin:from_codes_1d": lambda: AsymmetricBinaryIndex.from_codes(D["u8"][0]),
    }.items():
        out[f"new.{name}"] = f


def _from_packed_cases(out):
    def one(kind, cls, words, q):
        wide = np.concatenate([words, words[:, :1]], axis=1)
        for name, f in {
            "dtype": lambda: cls.from_packed(words.astype(np.int64), DIM, q), "1d": lambda: cls.from_packed(words[0], DIM, q),
            "3d": lambda: cls.from_packed(words[None], DIM, q), "dim_type": lambda: cls.from_packed(words, 11.0, q),
            "dim_0": lambda: cls.from_packed(words, 0, q), "dim_negative": lambda: cls.from_packed(words, -1, q),
            "dim_big": lambda: cls.from_packed(np.zeros((1, 257), np.uint32), 8193, q),
            "width": lambda: cls.from_packed(wide, DIM, q), "pad": lambda: cls.from_packed(_pad(words), DIM, q),
            "empty": lambda: cls.from_packed(words[:0], DIM, q), "quantizer_type": lambda: cls.from_packed(words, DIM, 3),
            "distance_type": lambda: cls.from_packed(words, DIM, q, "euclidean"),
            "dtype+1d": lambda: cls.from_packed(words[0].astype(np.int64), DIM, q),
            "dtype+dim_type": lambda: cls.from_packed(words.astype(np.int64), None, q),
            "1d+dim_0": lambda: cls.from_packed(words[0], 0, q), "dim_0+width": lambda: cls.from_packed(wide, 0, q),
            "width+pad": lambda: cls.from_packed(_pad(wide), DIM, q), "pad+quantizer_type": lambda: cls.from_packed(_pad(words), DIM, 3),
            "pad+empty": lambda: cls.from_packed(_pad(words)[:0], DIM, q),
            "width+quantizer_type": lambda: cls.from_packed(wide, DIM, 3),
        }.items():
            out[f"{kind}.from_packed:{name}"] = f

    one("bin", BinaryIndex, D["w1"], BQ)
    one("abin", AsymmetricBinaryIndex, D["w1"], BQ)
    one("sq4", Scalar4Index, D["w4"], SQ4)
    out["sq4.from_packed:levels"] = lambda: Scalar4Index.from_packed(D["w4"], DIM, SQ)
    out["sq4.from_packed:pad+levels"] = lambda: Scalar4Index.from_packed(_pad(D["w4"]), DIM, SQ)
    out["bin.from_packed:cosine"] = lambda: BinaryIndex.from_packed(D["w1"], DIM, BQ, Distance.cosine())
    out["bin.from_packed:pad+cosine"] = lambda: BinaryIndex.from_packed(_pad(D["w1"]), DIM, BQ, Distance.cosine())


def _call_cases():
    out = {}
    _constructor_cases(out)
    _from_packed_cases(out)
    above = D["c4"].copy()
    above[1, 2] = 16
    pq_above = D["pq"].copy()
    pq_above[1, 0] = K
    # -- the inverted files' adds
    for kind in ("ivfpq", "ivfpq_residual"):
        _ivf_add_cases(out, kind, "add_codes", D["pq"], np.float32, [("code_k", pq_above), ("code_negative", -D["pq"].astype(np.int64) - 1)])
    for kind in ("ivfflat", "ivfflat_f16"):
        _ivf_add_cases(out, kind, "add_rows", D["rows"], np.int32)
    for kind, codes, packed in (("ivfsq", D["u8"], None), ("ivfsq4", D["c4"], D["w4"]), ("ivfbin", D["u8"], D["w1"])):
        _ivf_add_cases(out, kind, "add_rows", D["rows"], np.int32)
        _ivf_add_cases(out, kind, "add_codes", codes, np.int64, [("above_15", above)] if kind == "ivfsq4" else ())
        if packed is not None:
            _ivf_add_cases(out, kind, "add_packed", packed, np.int32, [("pad", _pad(packed))])
    for kind in ("ivfpq", "ivfflat", "ivfsq", "ivfsq4", "ivfbin"):
        for name, X in (("3d", D["rows"][None]), ("width", D["rows"][:, :-1]), ("1d_width", D["rows"][0, :-1])):
            out[f"{kind}.add:{name}"] = (lambda kind=kind, X=X: _ivf(kind).add(X))
    # -- the resident indexes' adds
    _resident_add_cases(out, "flat", "add", D["rows"], np.float16)
    out["flat_f16.add:dtype"] = lambda: FlatIndex(D["rows"].astype(np.float16)).add(D["rows"])
    for kind, codes, packed in (("sq", D["u8"], None), ("sq4", D["c4"], D["w4"]), ("bin", D["u8"], D["w1"]), ("abin", D["u8"], D["w1"])):
        _resident_add_cases(out, kind, "add", D["rows"], np.float64)
        _resident_add_cases(out, kind, "add_codes", codes, np.int64, [("above_15", above)] if kind == "sq4" else ())
        _device_n_cases(out, kind, _resident, "add_device")
        if packed is not None:
            _resident_add_cases(out, kind, "add_packed", packed, np.int32, [("pad", _pad(packed))])
            _device_n_cases(out, kind, _resident, "add_packed_device")
        if kind in ("sq", "sq4"):
            _device_n_cases(out, kind, _resident, "add_codes_device")
    _device_n_cases(out, "flat", _resident, "add_device")
    # -- nq of every device-form call
    exact = [("search_device", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0)),
             ("search_device_masked", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0, dev_allowed=0)),
             ("range_search_device", lambda ix, nq: ix.range_search_device(0, nq, 1.0)),
             ("range_search_device_masked", lambda ix, nq: ix.range_search_device(0, nq, 1.0, dev_allowed=0))]
    for kind in ("flat", "sq", "sq4", "abin"):
        _nq_cases(out, kind, _resident, exact)
    _nq_cases(out, "bin", _resident, [
        ("search_device", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0)),
        ("hamming_range_search_device", lambda ix, nq: ix.hamming_range_search_device(0, nq, 1)),
        ("filtered_search_device", lambda ix, nq: ix.filtered_search_device(0, nq, 1, 0, 0, 0)),
        ("filtered_hamming_range_search_device", lambda ix, nq: ix.filtered_hamming_range_search_device(0, nq, 1, 0))])
    ivf_exact = [("search_device", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0, 2)),
                 ("search_device_masked", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0, 2, dev_allowed=0)),
                 ("range_search_device", lambda ix, nq: ix.range_search_device(0, nq, 1.0, 2)),
                 ("range_search_device_masked", lambda ix, nq: ix.range_search_device(0, nq, 1.0, 2, dev_allowed=0))]
    for kind in ("ivfflat", "ivfsq", "ivfsq4"):
        _nq_cases(out, kind, _ivf, ivf_exact)
    _nq_cases(out, "ivfpq", _ivf, [("search_device", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0, 2)),
                                   ("masked_search_device", lambda ix, nq: ix.masked_search_device(0, nq, 1, 0, 0, 0, 2))])
    _nq_cases(out, "ivfbin", _ivf, [
        ("search_device", lambda ix, nq: ix.search_device(0, nq, 1, 0, 0, 2)),
        ("hamming_range_search_device", lambda ix, nq: ix.hamming_range_search_device(0, nq, 1, 2)),
        ("filtered_search_device", lambda ix, nq: ix.filtered_search_device(0, nq, 1, 0, 0, 0, 2)),
        ("filtered_hamming_range_search_device", lambda ix, nq: ix.filtered_hamming_range_search_device(0, nq, 1, 0, 2))])
    # (nq after another fault: the earlier check answers)
    out["ivfsq.search_device:nq_negative+nprobe_0"] = lambda: _ivf("ivfsq").search_device(0, -1, 1, 0, 0, 0)
    out["ivfbin.hamming_range_search_device:nq_negative+radius"] = lambda: _ivf("ivfbin").hamming_range_search_device(0, -1, -1, 2)
    out["sq.search_device:nq_negative+topk_0"] = lambda: _resident("sq").search_device(0, -1, 0, 0, 0)
    out["ivfpq.masked_search_device:nq_negative+no_mask"] = lambda: _ivf("ivfpq").masked_search_device(0, -1, 1, 0, 0, None, 2)
    return out


# ---- corrupt files -----------------------------------------------------------------------------------------------------
# format: (class, a valid index, header struct, the fields' names in order, the blocks behind the header as (name, bytes),
# out-of-range values per field)

def _formats():
    w1, w4 = D["w1"].shape[1], D["w4"].shape[1]
    coarse, lists = ("coarse", NLIST * DIM * 4), ("lists", N * 4)
    u32 = 1 << 32
    inf, nan = float("inf"), float("nan")
    ivf_common = {"metric": [5, u32 - 1], "dim": [0, DIM + 1, DIM - 1], "nlist": [0, 65537, NLIST + 1, NLIST - 1], "n": [u32, N + 1, N - 1]}
    sqf = {"min": [5.0, nan, inf], "max": [-3.0, nan], "levels": [0, 1, 257]}
    sq4f = {"min": [5.0, nan], "max": [-3.0, inf], "levels": [0, 1, 17, 256, 257]}
    bqf = {"threshold": [nan, inf], "low": [256, 200, 201], "high": [256, 3, 2]}
    res_common = {"n": [0, u32, N + 1, N - 1], "metric": [5, u32 - 1]}
    return {
        "ivfpq": (IVFPQIndex, _ivf("ivfpq"), "<8sIIIIIIQ", ["magic", "metric", "dim", "nlist", "m", "k", "reserved", "n"],
                  [coarse, ("codebooks", M * K * DIM * 4), lists, ("payload", N * M)],
                  {**ivf_common, "metric": [3, 4, u32 - 1], "dim": [0, DIM + 1], "m": [0, 2, DIM], "k": [0, 65537, 38401, K - 1, K + 1, 257],
                   "reserved": [1]}),
        "ivfpq_residual": (IVFPQIndex, _ivf("ivfpq_residual"), "<8sIIIIIIQ", ["magic", "metric", "dim", "nlist", "m", "k", "reserved", "n"],
                           [coarse, ("codebooks", M * K * DIM * 4), lists, ("payload", N * M)], {"metric": [3], "reserved": [7], "n": [u32]}),
        "ivfflat": (IVFFlatIndex, _ivf("ivfflat"), "<8sIIIIQ", ["magic", "metric", "dim", "nlist", "dtype", "n"],
                    [coarse, lists, ("payload", N * DIM * 4)], {**ivf_common, "dtype": [1, 2, u32 - 1]}),
        "ivfflat_f16": (IVFFlatIndex, _ivf("ivfflat_f16"), "<8sIIIIQ", ["magic", "metric", "dim", "nlist", "dtype", "n"],
                        [coarse, lists, ("payload", N * DIM * 2)], {"dtype": [0, 2], "n": [N + 1]}),
        "ivfsq": (IVFScalarIndex, _ivf("ivfsq"), "<8sIIIffIQ", ["magic", "metric", "dim", "nlist", "min", "max", "levels", "n"],
                  [coarse, lists, ("payload", N * DIM)], {**ivf_common, **sqf}),
        "ivfsq4": (IVFScalar4Index, _ivf("ivfsq4"), "<8sIIIffIQ", ["magic", "metric", "dim", "nlist", "min", "max", "levels", "n"],
                   [coarse, lists, ("payload", N * w4 * 4)], {**ivf_common, **sq4f, "dim": [0, 9, 16, 17, 8]}),
        "ivfbin": (IVFBinaryIndex, _ivf("ivfbin"), "<8sIIIIfIIQ",
                   ["magic", "metric", "cmetric", "dim", "nlist", "threshold", "low", "high", "n"],
                   [coarse, lists, ("payload", N * w1 * 4)],
                   {**ivf_common, **bqf, "metric": [3, 4, u32 - 1], "cmetric": [5, u32 - 1], "dim": [0, 8193, 10, 33, 12]}),
        "sq": (ScalarIndex, _resident("sq"), "<8sQIIffI", ["magic", "n", "dim", "metric", "min", "max", "levels"],
               [("payload", N * DIM)], {**res_common, **sqf, "dim": [0, DIM + 1, DIM - 1]}),
        "sq4": (Scalar4Index, _resident("sq4"), "<8sQIIffI", ["magic", "n", "dim", "metric", "min", "max", "levels"],
                [("payload", N * w4 * 4)], {**res_common, **sq4f, "dim": [0, 9, 17, 8]}),
        "bin": (BinaryIndex, _resident("bin"), "<8sIIfIIQ", ["magic", "metric", "dim", "threshold", "low", "high", "n"],
                [("payload", N * w1 * 4)], {**res_common, **bqf, "metric": [3, 4, u32 - 1], "dim": [0, 8193, 10, 33]}),
        "abin": (AsymmetricBinaryIndex, _resident("abin"), "<8sQIIfII", ["magic", "n", "dim", "metric", "threshold", "low", "high"],
                 [("payload", N * w1 * 4)], {**res_common, **bqf, "dim": [0, 8193, 10, 33]}),
    }


def _file_bytes(ix) -> bytes:
    with tempfile.TemporaryDirectory() as d:
        ix.save(os.path.join(d, "f"))
        with open(os.path.join(d, "f"), "rb") as f:
            return f.read()


def _load(cls, raw: bytes):
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "f"), "wb") as f:
            f.write(raw)
        return cls.load(os.path.join(d, "f"))


def _file_cases():
    out = {}
    for fmt, (cls, ix, layout, fields, blocks, bad) in _formats().items():
        head = struct.Struct(layout)
        raw = _file_bytes(ix)
        assert len(raw) == head.size + sum(b for _, b in blocks), fmt
        values = list(head.unpack(raw[:head.size]))

        def add(name, data, cls=cls, fmt=fmt):
            out[f"file.{fmt}:{name}"] = lambda: _load(cls, data)

        add("empty", b"")
        add("short_header", raw[:head.size - 1])
        add("wrong_magic", b"VQNOTANY" + raw[8:])
        add("other_magic", (b"VQSQIDX1" if fmt != "sq" else b"VQBINIX1") + raw[8:])
        for field, bads in bad.items():
            for v in bads:
                changed = list(values)
                changed[fields.index(field)] = v
                add(f"{field}={v}", head.pack(*changed) + raw[head.size:])
        if "metric" in bad and "dim" in bad:  # two fields at once
            changed = list(values)
            changed[fields.index("metric")], changed[fields.index("dim")] = bad["metric"][0], 0
            add("metric+dim", head.pack(*changed) + raw[head.size:])
            add("wrong_magic+metric", b"VQNOTANY" + head.pack(*changed)[8:] + raw[head.size:])
        end = head.size
        starts = {}
        for name, size in blocks:
            starts[name] = end
            end += size
            add(f"{name}_short_one_byte", raw[:end - 1])
            add(f"{name}_missing", raw[:end - size])
        add("trailing_byte", raw + b"\0")
        if "lists" in starts:
            at = starts["lists"]
            add("list_id=nlist", raw[:at] + struct.pack("<I", NLIST) + raw[at + 4:])
            add("list_id=nlist+trailing_byte", raw[:at] + struct.pack("<I", NLIST) + raw[at + 4:] + b"\0")
        if fmt in ("ivfsq4", "ivfbin", "sq4", "bin", "abin"):  # the last byte of a row's last word: pad bits, pad nibbles
            add("pad_set", raw[:-1] + bytes([raw[-1] | 0x80]))
            add("pad_set+trailing_byte", raw[:-1] + bytes([raw[-1] | 0x80]) + b"\0")
            if "lists" in starts:
                at = starts["lists"]
                add("pad_set+list_id=nlist", raw[:at] + struct.pack("<I", NLIST) + raw[at + 4:-1] + bytes([raw[-1] | 0x80]))
        if fmt.startswith("ivfpq"):
            add("code=k", raw[:-1] + bytes([K]))
            at = starts["lists"]
            add("code=k+list_id=nlist", raw[:at] + struct.pack("<I", NLIST) + raw[at + 4:-1] + bytes([K]))
    return out


def cases():
    """id -> a call without arguments that is refused"""
    return {**_call_cases(), **_file_cases()}


def outcome(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001  (which exception is the recorded result)
        return [type(e).__name__, str(e)]
    return ["no exception", ""]


CASES = cases()
def _recorded():
    with open(GOLDEN) as f:
        return json.load(f)


RECORDED = {} if __name__ == "__main__" else _recorded()


def test_the_recorded_cases_are_the_table():
    assert sorted(RECORDED) == sorted(CASES)
    assert len(CASES) > 1000
    assert not [k for k, v in RECORDED.items() if v[0] in ("no exception", "FfiError")]


@pytest.mark.parametrize("case", sorted(CASES))
def test_refused_as_recorded(case):
    assert outcome(CASES[case]) == RECORDED[case]


if __name__ == "__main__":
    got = {k: outcome(f) for k, f in sorted(CASES.items())}
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(got), "cases;", sorted({v[0] for v in got.values()}))
    print("not refused:", [k for k, v in got.items() if v[0] in ("no exception", "FfiError")])
