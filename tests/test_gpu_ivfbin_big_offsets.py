"""The inverted-file binary index held to its statement on words on both sides of a 32-bit boundary (in the manner of
tests/test_gpu_ivfsq_big_offsets.py: the same helpers, tests/big_offsets.py, and the same skip rule).

n = 2^25 + 4099 rows of dim = 1024, 32 words or 128 bytes each (4.3 GB): the list-order word array crosses byte 2^31
(row 2^24) and byte 2^32 (row 2^25).  Two lists, rows [0, 2^22) and the rest, added in that order, so that list order is
row order and both boundaries fall inside the second list.  Every row has every bit set except planted rows, whose first
H bits are set and the rest clear; the query is below the threshold in every dimension, so the Hamming distance of a
planted row is its H and the result is the planted rows in (H, row) order (two of them tie).  The centroids put the query
nearer to the second list: nprobe 1 scans it alone, nprobe 2 both.

The expected distances come from the numpy statement (tests/ref_binary.py) over the planted rows; every unplanted row is
at H = 1024, farther than each of them (the one inequality here).  Each test states its device and host memory need and
skips with both numbers where either is short.  A run that counts as evidence shows no skips here."""
import numpy as np
import pytest

import big_offsets as BO
import ref_binary as B
from vq_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GiB = 1 << 30
SPLIT = 1 << 22
BQ = (0.0, 0, 3)


def _host_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def _need(dev_bytes, host_bytes, what):
    free, total = torch.cuda.mem_get_info()
    host = _host_available()
    if free < dev_bytes or host < host_bytes:
        pytest.skip(f"{what} needs {dev_bytes / GiB:.1f} GiB of device memory ({free / GiB:.1f} GiB of {total / GiB:.1f} free) "
                    f"and {host_bytes / GiB:.1f} GiB of host memory ({host / GiB:.1f} GiB available)")


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
    planted[first] = planted[first - 1]  # a tie: the lower row first
    planted[n - 1] = 0  # the last row is the nearest
    assert max(planted.values()) < hmax
    return planted


@pytest.mark.parametrize("metric", [B.MAN, B.EUC])
def test_search_words_past_byte_2e32(metric):
    n, d = (1 << 25) + 4099, 1024
    W = d // 32
    row_b = W * 4
    # device: the words in list order, ids, two queries' distances, slack; host: the index's words in add order (a vector
    # that doubles as it grows: up to three times its final size in flight) and one piece of 2^20 rows
    _need(n * row_b + n * 4 + 2 * n * 4 + 2 * GiB, 3 * n * row_b + 2 * GiB, "words of 128 bytes a row in list order")
    _lib.set_device(0)
    rows = BO.boundary_rows(n, W, 4, rows=False)
    assert any(r * row_b <= (1 << 31) < (r + 1) * row_b for r in rows.values())  # a planted row holds byte 2^31
    assert any(r * row_b <= (1 << 32) < (r + 1) * row_b for r in rows.values())  # ... and one byte 2^32
    assert min(rows.values()) - 1 >= SPLIT  # every boundary lies inside the second list
    planted = _plant(n, rows.values(), d)
    ids = np.array(sorted(planted), np.int64)
    pbits = np.zeros((len(ids), d), bool)
    for j, r in enumerate(ids):
        pbits[j, :planted[int(r)]] = True
    pwords = B.pack(pbits)
    q = np.full((2, d), -1.0, np.float32)  # every bit clear
    coarse = np.stack([np.full(d, 1, np.float32), np.full(d, 0.5, np.float32)])
    ix = _lib.IVFBin(coarse, BQ[0], BQ[1], BQ[2], metric, _lib.EUCLIDEAN)
    try:
        piece = 1 << 20
        for r0 in range(0, n, piece):
            r1 = min(n, r0 + piece)
            block = np.full((r1 - r0, W), 0xFFFFFFFF, np.uint32)
            inside = (ids >= r0) & (ids < r1)
            block[ids[inside] - r0] = pwords[inside]
            ix.add_packed((np.arange(r0, r1) >= SPLIT).astype(np.uint32), block)
        assert ix.list_sizes().tolist() == [SPLIT, n - SPLIT]
        assert ix.probe(q, 2).tolist() == [[1, 0], [1, 0]]
        topk = len(ids)
        H = B.hamming(B.pack(B.bits_f32(q[:1], BQ[0])), pwords)[0]
        assert np.all(H < d)  # every unplanted row (H = d) is farther than every planted one
        order = np.argsort(H, kind="stable")  # (H, row): ids ascends
        wi = ids[order].astype(np.uint32)
        wd = B.reported(d, BQ[1], BQ[2], metric)[H[order]]
        for nprobe in (1, 2):
            gi, gd = ix.search(q, nprobe, topk)
            assert np.array_equal(gi, np.stack([wi, wi])), f"boundaries {rows}, nprobe {nprobe}"
            assert np.array_equal(gd.view(np.uint32), np.stack([wd, wd]).view(np.uint32))
    finally:
        ix.close()
        torch.cuda.synchronize()
        _lib.synchronize()
        torch.cuda.empty_cache()
