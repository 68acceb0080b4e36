"""The inverted-file index files, byte for byte: a tiny deterministic index of each kind (IVFPQIndex plain and
residual, IVFFlatIndex in float32 and float16, IVFScalarIndex, IVFScalar4Index, IVFBinaryIndex), built with the host-only
add paths, is saved and the file's SHA-256 compared with the digest the same construction gave before the indexes came to
share one host layer; then loaded, and every array compared.  The ``*_handed`` kinds of the three classes that hand their
payload to the handle build the handle between the two adds and close it before saving: the same bytes.  No GPU."""
import hashlib

import numpy as np
import pytest

import vq_amd
from vq_amd import BinaryQuantizer, Distance, ScalarQuantizer
from vq_amd.binary import pack_bits

NLIST, DIM, N, M, K = 3, 8, 11, 2, 16
SQ4_DIM = 11  # dim % 8 != 0: the second word of a row has five pad nibbles (DIM % 32 != 0 already: pad bits)

# Recorded at commit cb45b16 ("Add IVFScalarIndex: exact search of SQ codes in the probed lists only"), the parent of
# the change that introduced vq_amd/_ivf_common.py, by running _build(kind).save() there.
SHA256 = {
    "pq": "31f9c228984c2a6d304baa6b5988e144d846dcff79ae9121a975c523140fc7b0",
    "pq_residual": "cd0cf4f94aa92a31c22ced41fef6a72f123d8c1b7fb9ee6b0ea9f5610bc8fb42",
    "flat_f32": "91e451ee148c17ae6293b1b773a345f01f3330eb90d8cd356471d9a7f7947452",
    "flat_f16": "9a53eb938e4dea6ba228fb0edfeac6a7cd2487275a96258f4084dafbbae3b238",
    "sq": "f9b1421db8aeff97ecb42cb63d8c4d3fbc3fde11a97efc5a99469711f9a0bcfa",
}
# Recorded at commit 1716bef ("Time encode stages from the kernels' dispatches; no exit marker"), the parent of the change
# that gave the inverted files one add front, one payload owner and one file skeleton, by running _build(kind).save()
# there.
SHA256.update({
    "sq4": "bf0c11216af6899fead284a4f927330c609c67143534ae765127fb421a407a3a",
    "bin": "9073072ebdfb435b40021bf68974bc976313bb1b1ec5d70b882ce8e20fd7da48",
})
HANDED = {"sq_handed": "sq", "sq4_handed": "sq4", "bin_handed": "bin"}  # the same bytes as the host-only construction


def _build(kind):
    rng = np.random.default_rng(20261017)
    coarse = rng.standard_normal((NLIST, DIM)).astype(np.float32)
    lists = rng.integers(0, NLIST, N).astype(np.uint32)
    rows = (rng.standard_normal((N, DIM)) * 3).astype(np.float32)
    cb = rng.standard_normal((M, K, DIM // M)).astype(np.float32)
    pq_codes = rng.integers(0, K, (N, M)).astype(np.uint8)
    sq_codes = rng.integers(0, 256, (N, DIM)).astype(np.uint8)
    sq4_coarse = rng.standard_normal((NLIST, SQ4_DIM)).astype(np.float32)  # (new draws follow the old ones)
    sq4_codes = rng.integers(0, 16, (N, SQ4_DIM)).astype(np.uint8)
    bits = rng.integers(0, 2, (N, DIM)).astype(bool)
    handed = kind in HANDED
    kind = HANDED.get(kind, kind)
    if kind in ("pq", "pq_residual"):
        ix = vq_amd.IVFPQIndex(coarse, cb, Distance.squared_euclidean(), residual=kind == "pq_residual")
        adds = [(ix.add_codes, pq_codes[:7]), (ix.add_codes, pq_codes[7:])]  # two adds: the appends are part of the construction
    elif kind in ("flat_f32", "flat_f16"):
        ix = vq_amd.IVFFlatIndex(coarse, Distance.cosine(), np.float32 if kind == "flat_f32" else np.float16)
        adds = [(ix.add_rows, rows[:7]), (ix.add_rows, rows[7:])]
    elif kind == "sq":
        ix = vq_amd.IVFScalarIndex(coarse, ScalarQuantizer(-3.0, 5.0, 17), Distance.manhattan())
        adds = [(ix.add_codes, sq_codes[:7]), (ix.add_codes, sq_codes[7:])]
    elif kind == "sq4":
        ix = vq_amd.IVFScalar4Index(sq4_coarse, ScalarQuantizer(-3.0, 5.0, 9), Distance.cosine())
        adds = [(ix.add_codes, sq4_codes[:7]), (ix.add_packed, ScalarQuantizer.pack4_codes(sq4_codes[7:]))]
    else:
        ix = vq_amd.IVFBinaryIndex(coarse, BinaryQuantizer(0.25, 3, 200), Distance.squared_euclidean(), Distance.cosine())
        adds = [(ix.add_codes, np.where(bits[:7], 200, 3).astype(np.uint8)), (ix.add_packed, pack_bits(bits[7:]))]
    adds[0][0](lists[:7], adds[0][1])
    if handed:
        ix._handle()  # host-only: the rows move into the handle
    adds[1][0](lists[7:], adds[1][1])
    if handed:
        ix.close()  # the payload comes back to the host
    return ix


def _payload(ix):
    if isinstance(ix, vq_amd.IVFFlatIndex):
        return ix.rows
    return ix.packed() if isinstance(ix, (vq_amd.IVFScalar4Index, vq_amd.IVFBinaryIndex)) else ix.codes


@pytest.mark.parametrize("kind", sorted(SHA256) + sorted(HANDED))
def test_file_bytes_and_round_trip(kind, tmp_path):
    ix = _build(kind)
    assert len(ix) == N and ix.list_sizes().sum() == N
    path = tmp_path / f"{kind}.ivf"
    ix.save(path)
    assert hashlib.sha256(path.read_bytes()).hexdigest() == SHA256[HANDED.get(kind, kind)]
    back = type(ix).load(path)
    assert type(back) is type(ix) and len(back) == N
    assert back.distance.metric == ix.distance.metric
    assert np.array_equal(back.coarse_centroids, ix.coarse_centroids) and back.coarse_centroids.dtype == np.float32
    assert np.array_equal(back.list_ids, ix.list_ids) and back.list_ids.dtype == np.uint32
    assert _payload(back).dtype == _payload(ix).dtype
    assert np.array_equal(_payload(back).view(np.uint8), _payload(ix).view(np.uint8))  # (bits: f16 rows included)
    if kind.startswith("pq"):
        assert np.array_equal(back.codebooks, ix.codebooks) and back.residual == ix.residual
    elif kind.startswith("flat"):
        assert back.dtype == ix.dtype
    elif kind.startswith("bin"):
        q, b = ix.quantizer, back.quantizer
        assert (np.float32(b.threshold), b.low, b.high) == (np.float32(q.threshold), q.low, q.high)
        assert back.coarse_distance.metric == ix.coarse_distance.metric != ix.distance.metric
    else:
        q, b = ix.quantizer, back.quantizer
        assert (b._min, b._max, b.levels) == (q._min, q._max, q.levels)
    again = tmp_path / f"{kind}.again"
    back.save(again)
    assert again.read_bytes() == path.read_bytes()
