"""The binary index held to its statement on rows on both sides of a 32-bit boundary (in the manner of
tests/test_gpu_big_offsets.py: the same windows and helpers, tests/big_offsets.py, and the same skip rule).

  * pack: the f32 input X (2^25 + 4099 rows x 128, 17 GB, generated on the device; synth_uniform_host regenerates any
    window of it) crosses element 2^32; the packed words of every window equal tests/ref_binary.py.
  * search over packed rows crossing byte 2^32 (W = 32 words a row, n = 2^25 + 4099): every row is all ones except
    planted rows, whose Hamming distance to the all-zero query is small and distinct (two of them tie); the result is
    the planted rows in (H, row) order.
  * search past row 2^31 (W = 1, n = 2^31 + 4099), planted the same way.

Each test states its device memory need and skips with both numbers where the device has less free.  A run that counts
as evidence shows no skips here."""
import numpy as np
import pytest

import big_offsets as BO
import ref_binary as R
from vq_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30
D = 128
NX = (1 << 25) + 4099
SEED = 7


def _need(nbytes, what):
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes / GiB:.1f} GiB of device memory; {free / GiB:.1f} GiB of {total / GiB:.1f} free")


def _sync():
    torch.cuda.synchronize()
    _lib.synchronize()


def test_pack_device_past_element_2e32():
    W = D // 32
    _need(NX * D * 4 + NX * W * 4 + GiB, "pack of X")
    _lib.set_device(0)
    ds = _lib.Dataset.synthetic(NX, D, seed=SEED)
    try:
        out = torch.empty((NX, W), dtype=torch.int32, device="cuda")
        _sync()
        _lib.check(_lib.load().vqhip_bq_pack_device(0.5, ds.device_ptr, NX, D, out.data_ptr()))
        _sync()
        rows = BO.boundary_rows(NX, D, 4)
        rows.update({f"words {b}": r for b, r in BO.boundary_rows(NX, W, 4, rows=False).items()})
        bad = []
        for r0, r1 in BO.windows(NX, rows.values()):
            want = R.pack(R.bits_f32(_lib.synth_uniform_host(r1 - r0, D, SEED, r0), 0.5))
            got = out[r0:r1].cpu().numpy().view(np.uint32)
            bad += [r0 + int(i) for i in np.nonzero((got != want).any(axis=1))[0][:4]]
        assert not bad, f"packed rows that differ from tests/ref_binary.py: {bad} (boundaries {rows})"
        del out
    finally:
        ds.close()
        _sync()
        torch.cuda.empty_cache()


def _planted_search(n, d, planted, topk):
    """every row all ones except `planted` {row: H}, whose first H bits are one and the rest zero; searched with the
    all-zero query under Manhattan (D = H); returns (got, want)"""
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
        got = ix.search(q, topk)
        # every unplanted row has H = d, larger than every planted H
        order = sorted(planted.items(), key=lambda kv: (kv[1], kv[0]))[:topk]
        want_idx = np.array([[r for r, _ in order]] * 2, np.uint32)
        want_dist = np.array([[float(h) for _, h in order]] * 2, np.float32)
    finally:
        ix.close()
        del words
        _sync()
        torch.cuda.empty_cache()
    return got, (want_idx, want_dist)


def _plant(n, rows):
    """distinct small H per boundary row and its neighbours; rows r - 1 and r of the first boundary tie"""
    planted = {}
    h = 1
    for r in sorted(set(rows)):
        for rr in (r - 1, r, r + 1):
            if 0 <= rr < n and rr not in planted:
                planted[rr] = h
                h += 1
    first = sorted(set(rows))[0]
    if first - 1 >= 0 and first < n:
        planted[first] = planted[first - 1]  # a tie: the lower row first
    planted[n - 1] = 0  # the last row is the nearest
    return planted


def test_search_packed_rows_past_byte_2e32():
    n, d = NX, 1024
    _need(2 * n * 128 + 2 * GiB, "packed rows of 128 bytes, twice (the caller's and the index's copy)")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, d // 32, 4, rows=False)
    planted = _plant(n, rows.values())
    topk = len(planted)
    (gi, gd), (wi, wd) = _planted_search(n, d, planted, topk)
    assert np.array_equal(gi, wi), f"boundaries {rows}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def test_search_past_row_2e31():
    n, d = (1 << 31) + 4099, 32
    _need(2 * n * 4 + 2 * GiB, "packed rows of 4 bytes, twice (the caller's and the index's copy)")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, 1, 4)
    planted = _plant(n, rows.values())
    topk = len(planted)
    assert max(planted.values()) < d
    (gi, gd), (wi, wd) = _planted_search(n, d, planted, topk)
    assert np.array_equal(gi, wi), f"boundaries {rows}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
