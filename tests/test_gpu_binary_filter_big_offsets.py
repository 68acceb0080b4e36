"""The filtered binary search held to its statement on rows on both sides of a 32-bit boundary (in the manner of
tests/test_gpu_binary_big_offsets.py: its helpers, its planted rows and its skip rule).

  * masked search over packed rows crossing byte 2^32 (W = 32 words a row, n = 2^25 + 4099)
  * masked search past row 2^31 (W = 1, n = 2^31 + 4099)

Every row is all ones except planted rows around each boundary, whose Hamming distance to the all-zero query is small.
The mask allows every other planted row -- rows on each side of every boundary -- and nothing else: the result is those
rows in (H, row) order, then padding.  The masked scan skips every 64-row group without a planted row, so a test's time is
its construction's.

Each test states its device memory need and skips with both numbers where the device has less free.  A run that counts
as evidence shows no skips here."""
import numpy as np
import pytest

import big_offsets as BO
import ref_binary as R
import test_gpu_binary_big_offsets as T
from vq_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30


def _masked_planted_search(n, d, planted, allowed_rows, topk):
    """T._planted_search under the row mask that allows `allowed_rows` only; returns (got, want)"""
    W = (d + 31) // 32
    words = torch.full((n, W), -1, dtype=torch.int32, device="cuda")
    for r, h in planted.items():
        row_bits = np.zeros((1, d), bool)
        row_bits[0, :h] = True
        words[r] = torch.from_numpy(R.pack(row_bits)[0].view(np.int32)).cuda()
    T._sync()
    mask = np.zeros((n + 31) // 32, np.uint32)
    for r in allowed_rows:
        mask[r >> 5] |= np.uint32(1 << (r & 31))
    ix = _lib.Binary(None, _lib.BINARY_PACKED, n, d, 0.0, 0, 1, _lib.MANHATTAN, dev_src=words.data_ptr())
    try:
        q = np.full((2, d), -1.0, np.float32)  # all bits 0
        got = ix.search_masked(q, topk, mask)
        order = sorted(((planted[r], r) for r in allowed_rows))[:topk]
        want_idx = np.full((2, topk), 0xFFFFFFFF, np.uint32)
        want_dist = np.full((2, topk), np.inf, np.float32)
        want_idx[:, :len(order)] = [r for _, r in order]
        want_dist[:, :len(order)] = [float(h) for h, _ in order]
    finally:
        ix.close()
        del words
        T._sync()
        torch.cuda.empty_cache()
    return got, (want_idx, want_dist)


def _check(n, d, rows):
    planted = T._plant(n, rows.values())
    assert max(planted.values()) < d
    allowed = sorted(planted)[::2]  # every other planted row: one or two of the three around each boundary
    first = min(rows.values())
    assert any(r < first for r in allowed) and any(r >= max(rows.values()) for r in allowed)  # both sides
    topk = len(planted)  # more than the allowed rows: padding behind them
    (gi, gd), (wi, wd) = _masked_planted_search(n, d, planted, allowed, topk)
    assert np.array_equal(gi, wi), f"boundaries {rows}: {gi[0]} != {wi[0]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def test_masked_search_packed_rows_past_byte_2e32():
    n, d = T.NX, 1024
    T._need(2 * n * 128 + 2 * GiB, "packed rows of 128 bytes, twice (the caller's and the index's copy)")
    _lib.set_device(0)
    _check(n, d, BO.boundary_rows(n, d // 32, 4, rows=False))


def test_masked_search_past_row_2e31():
    n, d = (1 << 31) + 4099, 32
    T._need(2 * n * 4 + 2 * GiB + (n // 8), "packed rows of 4 bytes, twice (the caller's and the index's copy), and the mask")
    _lib.set_device(0)
    _check(n, d, BO.boundary_rows(n, 1, 4))
