"""The Hamming-radius range search of the binary index held to its statement on rows on both sides of a 32-bit boundary
(in the manner of tests/test_gpu_binary_big_offsets.py: the same skip rule, the same planting and the same two shapes).

  * packed rows crossing byte 2^32 (W = 32 words a row, n = 2^25 + 4099): every row is all ones except planted rows,
    whose Hamming distance to the all-zero query is small; the radius is the largest planted H, and the result is exactly
    the planted rows, in row order, with their H as the distance under Manhattan.
  * rows past 2^31 (W = 1, n = 2^31 + 4099), planted the same way: the batch is one query, the counts 2^18 entries.

Each test states its device memory need and skips with both numbers where the device has less free.  A run that counts
as evidence shows no skips here."""
import numpy as np
import pytest

import big_offsets as BO
import ref_binary as R
from test_gpu_binary_big_offsets import NX, GiB, _need, _plant, _sync
from vq_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _planted_range(n, d, planted):
    """every row all ones except `planted` {row: H}, whose first H bits are one and the rest zero; two all-zero queries
    under Manhattan (D = H), the first with the largest planted H as its radius and the second with the median one;
    returns (got, want)"""
    W = (d + 31) // 32
    words = torch.full((n, W), -1, dtype=torch.int32, device="cuda")
    for r, h in planted.items():
        row_bits = np.zeros((1, d), bool)
        row_bits[0, :h] = True
        row = R.pack(row_bits)[0]
        words[r] = torch.from_numpy(row.view(np.int32)).cuda()
    _sync()
    ix = _lib.Binary(None, _lib.BINARY_PACKED, n, d, 0.0, 0, 1, _lib.MANHATTAN, dev_src=words.data_ptr())
    try:
        q = np.full((2, d), -1.0, np.float32)  # all bits 0
        hs = sorted(planted.values())
        radii = np.array([hs[-1], hs[len(hs) // 2]], np.uint32)
        assert radii[0] < d  # every unplanted row has H = d: outside both radii
        got = ix.hamming_range_search(q, radii, 1 << 20).read()
        per = [[r for r in sorted(planted) if planted[r] <= int(h)] for h in radii]
        want = (np.array([0, len(per[0]), len(per[0]) + len(per[1])], np.uint64),
                np.array(per[0] + per[1], np.uint32), np.array([float(planted[r]) for r in per[0] + per[1]], np.float32))
    finally:
        ix.close()
        del words
        _sync()
        torch.cuda.empty_cache()
    return got, want


def _check(got, want, rows):
    assert np.array_equal(got[0], want[0]), f"boundaries {rows}"
    assert np.array_equal(got[1], want[1]), f"boundaries {rows}"
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


def test_range_packed_rows_past_byte_2e32():
    n, d = NX, 1024
    _need(2 * n * 128 + 2 * GiB, "packed rows of 128 bytes, twice (the caller's and the index's copy)")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, d // 32, 4, rows=False)
    planted = _plant(n, rows.values())
    _check(*_planted_range(n, d, planted), rows)


def test_range_past_row_2e31():
    n, d = (1 << 31) + 4099, 32
    _need(2 * n * 4 + 2 * GiB, "packed rows of 4 bytes, twice (the caller's and the index's copy)")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, 1, 4)
    planted = _plant(n, rows.values())
    assert max(planted.values()) < d
    _check(*_planted_range(n, d, planted), rows)
