"""The scalar index held to its statement on rows on both sides of a 32-bit boundary (in the manner of
tests/test_gpu_binary_big_offsets.py: the same helpers, tests/big_offsets.py, and the same skip rule).

  * codes crossing byte 2^32 (n = 2^25 + 4099 rows of d = 128 bytes, 4.3 GB): every row is code 255 in every dimension
    except planted rows, whose first H dimensions are 255 and the rest 0; against the query v(0) in every dimension the
    distance grows with H, so the result is the planted rows in (H, row) order (two of them tie).
  * rows past 2^31 at d = 1 (n = 2^31 + 4099): planted rows hold the code H, every other row 255.

The expected distances come from the numpy statement (tests/ref_sqindex.py) over the planted rows; every unplanted row
is farther than each of them.  Each test states its device memory need and skips with both numbers where the device has
less free.  A run that counts as evidence shows no skips here."""
import numpy as np
import pytest

import big_offsets as BO
import ref_knn as K
import ref_sqindex as R
from vq_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30
SQ = (-1.0, 1.0, 256)


def _need(nbytes, what):
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes / GiB:.1f} GiB of device memory; {free / GiB:.1f} GiB of {total / GiB:.1f} free")


def _sync():
    torch.cuda.synchronize()
    _lib.synchronize()


def _plant(n, rows, hmax):
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
    assert max(planted.values()) < hmax
    return planted


def _planted_search(n, d, row_of, planted, metric):
    """codes [n][d] all 255 except row r = row_of(H) for (r, H) in planted, searched with the query v(0) twice over;
    returns (got, want)"""
    codes = torch.full((n, d), 255, dtype=torch.uint8, device="cuda")
    ids = np.array(sorted(planted), np.int64)
    rows = np.stack([row_of(planted[int(r)]) for r in ids])
    for r, row in zip(ids, rows):
        codes[int(r)] = torch.from_numpy(row).cuda()
    _sync()
    ix = _lib.SQIndex(None, False, n, d, SQ[0], SQ[1], SQ[2], metric, dev_src=codes.data_ptr())
    try:
        del codes  # the index keeps its own copy
        _sync()
        torch.cuda.empty_cache()
        q = np.tile(R.decode(SQ, np.zeros(d, np.uint8)), (2, 1))
        topk = len(ids)
        got = ix.search(q, topk)
        dp = R.distances(metric, q[0], SQ, rows)
        far = R.distances(metric, q[0], SQ, np.full((1, d), 255, np.uint8))[0]
        assert np.all(dp < far)  # every unplanted row is farther than every planted one
        wi, wd = K.topk_of(dp, ids, topk)
        want = (np.stack([wi, wi]), np.stack([wd, wd]))
    finally:
        ix.close()
        _sync()
        torch.cuda.empty_cache()
    return got, want


@pytest.mark.parametrize("metric", [K.MANHATTAN, K.EUCLIDEAN])
def test_search_codes_past_byte_2e32(metric):
    n, d = (1 << 25) + 4099, 128
    _need(2 * n * d + 2 * n * 4 + 2 * GiB, "codes of 128 bytes a row, twice (the caller's and the index's copy), and two queries' distances")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, d, 1, rows=False)
    assert any(r * d <= (1 << 32) < (r + 1) * d for r in rows.values())  # a planted row holds byte 2^32
    planted = _plant(n, rows.values(), d)

    def row_of(h):
        row = np.zeros(d, np.uint8)
        row[:h] = 255
        return row

    (gi, gd), (wi, wd) = _planted_search(n, d, row_of, planted, metric)
    assert np.array_equal(gi, wi), f"boundaries {rows}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def test_search_past_row_2e31():
    n, d = (1 << 31) + 4099, 1
    _need(2 * n + n * 4 + 2 * GiB, "codes of one byte a row, twice (the caller's and the index's copy), and one query's distances")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, 1, 1)
    assert (1 << 31) in rows.values()
    planted = _plant(n, rows.values(), 255)
    (gi, gd), (wi, wd) = _planted_search(n, d, lambda h: np.array([h], np.uint8), planted, K.MANHATTAN)
    assert np.array_equal(gi, wi), f"boundaries {rows}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
