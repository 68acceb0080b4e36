"""What tests/test_ivf_mutate_host.py and tests/test_gpu_ivf_mutate.py share: the four inverted-file indexes at payload
widths that take every unit of the take kernel (16, 4 and 1 bytes), their rows as the add paths that need no device take
them, and the one statement of a removal (include/vqhip.h, "removing rows from an inverted file"): after any sequence of
adds and removals an index equals a fresh one given ``L'``, ``R'`` -- ref_mutate's ``kept`` applied to the list ids and the
rows together -- in one add."""
from __future__ import annotations

import numpy as np

from vq_amd import (BinaryQuantizer, Distance, IVFBinaryIndex, IVFFlatIndex, IVFPQIndex, IVFScalarIndex, ScalarQuantizer)
from vq_amd.binary import pack_bits

F = np.float32
SQ = ScalarQuantizer(-3.0, 3.0, 256)
BQ = BinaryQuantizer(0.0)
NLIST = 5
EMPTY_LIST = 3  # no row is ever put there
SUB_DIM = 4     # of the PQ kinds

# name -> (family, metric, shape): flat (dtype, d), sq d, bin d, pq (m, k, residual); the comment is the payload's row width
KINDS = {
    "flat32_d21": ("flat", "euclidean", (np.float32, 21)),            # 84 bytes: 4-byte units
    "flat32_d128": ("flat", "squared_euclidean", (np.float32, 128)),  # 512: 16-byte units
    "flat16_d21": ("flat", "manhattan", (np.float16, 21)),            # 42: byte units
    "flat32_d21_cos": ("flat", "cosine", (np.float32, 21)),           # the norms move too
    "flat16_d21_cos": ("flat", "cosine", (np.float16, 21)),
    "sq_d1": ("sq", "manhattan", 1),                                  # 1
    "sq_d21": ("sq", "euclidean", 21),                                # 21
    "sq_d21_cos": ("sq", "cosine", 21),
    "bin_d20": ("bin", "manhattan", 20),                              # one word, pad bits
    "bin_d96": ("bin", "manhattan", 96),                              # 12 bytes
    "bin_d1024": ("bin", "euclidean", 1024),                          # 128: 16-byte units
    "pq_m2_k16": ("pq", "euclidean", (2, 16, False)),                 # 2
    "pq_m8_k16": ("pq", "squared_euclidean", (8, 16, False)),         # 8
    "pq_m3_k300": ("pq", "manhattan", (3, 300, False)),               # u16 codes: 6
    "pq_m2_k16_res": ("pq", "euclidean", (2, 16, True)),
    "pq_m8_k16_res": ("pq", "euclidean", (8, 16, True)),
    "pq_m3_k300_res": ("pq", "squared_euclidean", (3, 300, True)),
}
ONE_PER_INDEX = ["flat32_d21_cos", "sq_d21", "bin_d96", "pq_m3_k300_res"]


def family(kind):
    return KINDS[kind][0]


def dim(kind):
    fam, _, shape = KINDS[kind]
    return {"flat": lambda: shape[1], "sq": lambda: shape, "bin": lambda: shape, "pq": lambda: shape[0] * SUB_DIM}[fam]()


def coarse(kind):
    return np.random.default_rng(1000 + dim(kind)).standard_normal((NLIST, dim(kind))).astype(F)


def make(kind):
    """an index of the kind without rows"""
    fam, metric, shape = KINDS[kind]
    c = coarse(kind)
    if fam == "flat":
        return IVFFlatIndex(c, Distance(metric), shape[0])
    if fam == "sq":
        return IVFScalarIndex(c, SQ, Distance(metric))
    if fam == "bin":
        return IVFBinaryIndex(c, BQ, Distance(metric))
    m, k, residual = shape
    cb = np.random.default_rng(2000 + m * k).standard_normal((m, k, SUB_DIM)).astype(F)
    return IVFPQIndex(c, cb, Distance(metric), residual=residual)


def gen(kind, seed, b):
    """(list ids (b,), payload (b, w)) of b rows: no row in EMPTY_LIST, and rows 30 .. 39 are rows 10 .. 19 again, in the
    same lists (ties by row id)"""
    fam, _, shape = KINDS[kind]
    rng = np.random.default_rng(seed)
    lists = rng.choice([l for l in range(NLIST) if l != EMPTY_LIST], b).astype(np.uint32)
    if fam == "flat":
        rows = rng.standard_normal((b, shape[1])).astype(shape[0])
    elif fam == "sq":
        rows = rng.integers(0, 256, (b, shape), dtype=np.uint8)
    elif fam == "bin":
        rows = pack_bits(rng.standard_normal((b, shape)) >= 0.0)
    else:
        rows = rng.integers(0, shape[1], (b, shape[0])).astype(np.uint8 if shape[1] <= 256 else np.uint16)
    if b >= 40:
        lists[30:40], rows[30:40] = lists[10:20], rows[10:20]
    return lists, np.ascontiguousarray(rows)


def add(ix, kind, lists, rows):
    """the add path of the kind that needs no device"""
    fam = family(kind)
    if fam == "flat":
        return ix.add_rows(lists, rows)
    if fam == "bin":
        return ix.add_packed(lists, rows)
    return ix.add_codes(lists, rows)


def stored(ix, kind):
    fam = family(kind)
    return ix.rows if fam == "flat" else ix.packed() if fam == "bin" else ix.codes


def fresh(kind, lists, rows):
    ix = make(kind)
    if lists.shape[0]:
        add(ix, kind, lists, rows)
    return ix


def file_bytes(ix, tmp_path, name):
    p = tmp_path / name
    ix.save(p)
    return p.read_bytes()


def same_host_state(kind, ix, lists, rows, what, tmp_path=None):
    """everything the statement says of the calls that need no device"""
    want = fresh(kind, lists, rows)
    n = lists.shape[0]
    assert len(ix) == n, f"{what}: len {len(ix)}, want {n}"
    assert ix.list_ids.dtype == np.uint32 and np.array_equal(ix.list_ids, lists), f"{what}: list_ids differ"
    assert np.array_equal(ix.list_sizes(), want.list_sizes()), f"{what}: list_sizes() differ"
    got = stored(ix, kind)
    assert got.dtype == rows.dtype and got.shape == rows.shape and np.array_equal(got.view(np.uint8), rows.view(np.uint8)), \
        f"{what}: the stored rows differ"
    if ix._ix is not None:
        assert np.array_equal(ix._ix.list_sizes(), want.list_sizes()), f"{what}: the handle's list_sizes differ"
        assert ix._ix.info()[0] == n, f"{what}: the handle's n is {ix._ix.info()[0]}, want {n}"
    if tmp_path is not None:
        assert file_bytes(ix, tmp_path, "got") == file_bytes(want, tmp_path, "want"), f"{what}: the saved files differ"
    return want
