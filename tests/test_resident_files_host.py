"""The four resident-index files, byte for byte: a tiny deterministic ScalarIndex (from codes), BinaryIndex and
AsymmetricBinaryIndex (from packed words and from u8 codes, d % 32 != 0 so that the last word has pad bits) and
Scalar4Index (from codes and from packed words, d % 8 != 0: pad nibbles) is saved and the file's SHA-256 compared with
the digest the same construction gave before the resident indexes came to share one host layer; then loaded, and
every field and array compared.  Nothing here reaches the device.  No GPU."""
import hashlib

import numpy as np
import pytest

from vq_amd import AsymmetricBinaryIndex, BinaryIndex, BinaryQuantizer, Distance, Scalar4Index, ScalarIndex, ScalarQuantizer
from vq_amd.binary import pack_bits, words_per_row

N, SQ_DIM, BIN_DIM, SQ4_DIM = 11, 8, 40, 11

# Recorded at commit b57b196 ("Encode sub_dim 16 on three bf16 products at two waves per SIMD"), the parent of the change
# that introduced vq_amd/_resident_common.py, by running _build(kind).save() there.
SHA256 = {
    "sq_codes": "6c87d7b9017d7561341553f48bbcd76b045c30e7a1f5a9e9dc4db04466349bc4",
    "bin_packed": "6f7d7ee80907efbe1f02192a8927fa74a99062a65f2de72951cb797c71b54da6",
    "bin_codes": "e6717da2f46d41654972c0434aef15c7df8c8f29147fc1ba8da46926a4ccbf81",
}
# Recorded at commit 1716bef ("Time encode stages from the kernels' dispatches; no exit marker"), the parent of the change
# that gave the four resident files one reader and writer, by running _build(kind).save() there.
SHA256.update({
    "sq4_codes": "81798fba98d52dee06594ba1be66641474628e4a362dab1b984f38f5dca99a9e",
    "sq4_packed": "77eb8aeeb17c3b468ed6273d810c4ff5cd8b8c5179011dfa3bc63108d442eea3",
    "abin_packed": "72ee1cac5191c28f4dbdda5c1190e84e9a8dcc7d5ba52faf9eb1ddbb2c037019",
    "abin_codes": "8549d4baba75d5d55a1f4591c9348eccf8aec9cdd2e061fbaabc90d3eecd7514",
})


def _build(kind):
    rng = np.random.default_rng(20261017)
    sq_codes = rng.integers(0, 256, (N, SQ_DIM)).astype(np.uint8)
    bits = rng.integers(0, 2, (N, BIN_DIM)).astype(bool)
    bq = BinaryQuantizer(0.25, 3, 200)
    if kind == "sq_codes":
        return ScalarIndex.from_codes(sq_codes, ScalarQuantizer(-3.0, 5.0, 17), Distance.manhattan())
    if kind == "bin_packed":
        return BinaryIndex.from_packed(pack_bits(bits), BIN_DIM, bq, Distance.euclidean())
    if kind == "bin_codes":
        return BinaryIndex.from_codes(np.where(bits, 200, 3).astype(np.uint8), bq, Distance.squared_euclidean())
    sq4_codes = rng.integers(0, 16, (N, SQ4_DIM)).astype(np.uint8)  # (new draws follow the old ones)
    sq4 = ScalarQuantizer(-3.0, 5.0, 9)
    if kind == "sq4_codes":
        return Scalar4Index.from_codes(sq4_codes, sq4, Distance.cosine())
    if kind == "sq4_packed":
        return Scalar4Index.from_packed(ScalarQuantizer.pack4_codes(sq4_codes), SQ4_DIM, sq4, Distance.manhattan())
    if kind == "abin_packed":
        return AsymmetricBinaryIndex.from_packed(pack_bits(bits), BIN_DIM, bq, Distance.cosine())
    return AsymmetricBinaryIndex.from_codes(np.where(bits, 200, 3).astype(np.uint8), bq, Distance.euclidean())


def _dim(kind):
    return SQ_DIM if kind == "sq_codes" else SQ4_DIM if kind.startswith("sq4") else BIN_DIM


def _payload(ix):
    if isinstance(ix, Scalar4Index):
        return ix.packed()
    return ix.codes() if isinstance(ix, ScalarIndex) else ix._host_words()


@pytest.mark.parametrize("kind", sorted(SHA256))
def test_file_bytes_and_round_trip(kind, tmp_path):
    ix = _build(kind)
    dim = _dim(kind)
    assert len(ix) == N and ix.dim == dim and ix._ix is None
    path = tmp_path / f"{kind}.idx"
    ix.save(path)
    assert ix._ix is None
    assert hashlib.sha256(path.read_bytes()).hexdigest() == SHA256[kind]
    back = type(ix).load(path)
    assert type(back) is type(ix) and len(back) == N and back.dim == dim and back._ix is None
    assert back.distance.metric == ix.distance.metric
    q, b = ix.quantizer, back.quantizer
    if kind == "sq_codes":
        assert (b._min, b._max, b.levels) == (q._min, q._max, q.levels)
        assert _payload(back).dtype == np.uint8 and _payload(back).shape == (N, dim)
    elif kind.startswith("sq4"):
        assert (b._min, b._max, b.levels) == (q._min, q._max, q.levels)
        assert _payload(back).dtype == np.uint32 and _payload(back).shape == (N, (dim + 7) // 8)
        assert np.array_equal(back.codes(), ix.codes()) and back.codes().shape == (N, dim)
    else:
        assert (np.float32(b.threshold), b.low, b.high) == (np.float32(q.threshold), q.low, q.high)
        assert _payload(back).dtype == np.uint32 and _payload(back).shape == (N, words_per_row(dim))
    assert np.array_equal(_payload(back), _payload(ix))
    again = tmp_path / f"{kind}.again"
    back.save(again)
    assert again.read_bytes() == path.read_bytes()
    assert ix._ix is None and back._ix is None


def test_the_two_binary_sources_pack_to_the_same_words():
    """u8 codes (bit = code >= high) and the packed words of the same bits give the same rows, pad bits zero"""
    packed, codes = _build("bin_packed")._host_words(), _build("bin_codes")._host_words()
    assert np.array_equal(packed, codes)
    assert not (packed[:, -1] >> np.uint32(BIN_DIM % 32)).any()
    assert np.array_equal(_build("abin_packed")._host_words(), packed)
    assert np.array_equal(_build("abin_codes")._host_words(), packed)
    assert np.array_equal(_build("sq4_codes").packed(), _build("sq4_packed").packed())
