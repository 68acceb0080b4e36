"""Removing rows from an inverted-file index whose device state is current (include/vqhip.h, "removing rows from an
inverted file"; vq_amd/csrc/k_ivf_remove.hip) on one MI355X, against what there was before and against the floor.

Three indexes of 1M rows in 1024 lists: IVFFlat over 128 x f32 (512 B a row), IVFPQ with m = 8, k = 256 (8 B a row) and
IVFBin over 1024 bits (128 B a row).  Four removals: a random 10 %, a random 50 %, the contiguous first 10 % and one whole
list.  Per line
  (i)   remove       the C call on a handle that has been searched, by wall clock (it returns synchronised).  It contains
                     host work, so it is split: `host_twin` is the same call on a handle that holds the same rows and was
                     never searched -- the mask walk and the in-place compaction of the host rows, no device -- and
                     `device_by_difference` = remove - host_twin: an ESTIMATE of the device part (upload of the mask and the
                     prefix, the view, the two kernels, the allocations and the synchronise).  The kernels are not timed
                     here: a kernel trace is a run of its own (profiles/ivf_mutate/kernel_times.json).  `uploads` must
                     not move across the call.
  (ii)  fresh        what the parent offers: a new handle, one add of the surviving rows, and the first search's upload,
                     by wall clock.
  (iii) memcpy       a device-to-device copy of the surviving payload bytes, the floor of the device part, taken the
                     cross-checked way tools/mutate_time.py takes it (three timings side by side; `ms` is None where they
                     disagree or beat the HBM peak).
The legs of one line are alternated in one process; the median of --reps with its extremes.  A removal changes the index,
so every repetition starts from a handle built and searched again (not timed).

    python tools/ivf_mutate_time.py [--reps 5] [--rows 1000000] [--out profiles/ivf_mutate/time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mutate_time import copy_floor, floor_stats, stats  # noqa: E402
from vq_amd import _lib  # noqa: E402

NLIST, DIM, NPROBE, TOPK = 1024, 128, 8, 10


def clock(fn):
    """milliseconds of fn() by wall clock, the device idle before and synchronised behind it"""
    _lib.synchronize()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    _lib.synchronize()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


class Case:
    """one index kind: its payload on the host, how a handle is made and filled"""

    def __init__(self, name, n, rng):
        self.name, self.n = name, n
        self.coarse = rng.standard_normal((NLIST, DIM)).astype(np.float32)
        self.lists = rng.integers(0, NLIST, n).astype(np.uint32)
        self.q = self.coarse[:4].copy()
        if name == "ivfflat":
            self.rb = 512
            self.rows = rng.standard_normal((n, DIM)).astype(np.float32)
        elif name == "ivfpq":
            self.rb = 8
            self.codebooks = rng.standard_normal((8, 256, DIM // 8)).astype(np.float32)
            self.rows = rng.integers(0, 256, (n, 8), dtype=np.uint8)
        else:
            self.rb = 128
            self.rows = rng.integers(0, 1 << 32, (n, DIM * 8 // 32), dtype=np.uint64).astype(np.uint32)

    def filled(self, lists, rows):
        if self.name == "ivfflat":
            h = _lib.IVFFlat(self.coarse, _lib.EUCLIDEAN)
            h.add(lists, rows)
        elif self.name == "ivfpq":
            h = _lib.IVFPQ(self.coarse, self.codebooks, _lib.EUCLIDEAN)
            h.add(lists, rows)
        else:
            h = _lib.IVFBin(np.ascontiguousarray(np.tile(self.coarse, (1, 8))), 0.0, 0, 1, _lib.MANHATTAN, _lib.EUCLIDEAN)
            h.add_packed(lists, rows)
        return h

    def search(self, h):
        q = self.q if self.name != "ivfbin" else np.ascontiguousarray(np.tile(self.q, (1, 8)))
        return h.search(q, NPROBE, TOPK)


def removal(case, label, m, reps):
    n, rb = case.n, case.rb
    words = np.packbits(m, bitorder="little")
    words = np.concatenate([words, np.zeros((-len(words)) % 4, np.uint8)]).view(np.uint32).copy()
    gone = int(m.sum())
    kept_bytes = (n - gone) * rb
    l2, r2 = np.ascontiguousarray(case.lists[~m]), np.ascontiguousarray(case.rows[~m])
    src = torch.empty(n * rb, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(max(kept_bytes, 16), dtype=torch.uint8, device="cuda")
    t_remove, t_host, t_fresh, t_next = [], [], [], []
    t_copy = {"events": [], "wall": [], "torch_events": []}
    want = None
    for _ in range(reps):
        h = case.filled(case.lists, case.rows)
        case.search(h)
        assert h.uploads() == 1
        t_remove.append(clock(lambda: h.remove(words)))
        assert h.uploads() == 1 and h.info()[0] == n - gone, "the removal left the device path"
        got = [None]
        t_next.append(clock(lambda: got.__setitem__(0, case.search(h))))
        assert h.uploads() == 1
        h.close()
        cold = case.filled(case.lists, case.rows)  # never searched: the host path
        t_host.append(clock(lambda: cold.remove(words)))
        assert cold.uploads() == 0
        cold.close()
        copy_floor(scratch, src, kept_bytes, t_copy)
        f = [None]

        def fresh():
            f[0] = case.filled(l2, r2)
            want_now = case.search(f[0])
            f.append(want_now)

        t_fresh.append(clock(fresh))
        want = f[1]
        f[0].close()
        assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1].view(np.uint32), want[1].view(np.uint32)), \
            "the removal and the fresh index disagree"
    line = {"index": case.name, "mask": label, "n": n, "nlist": NLIST, "row_bytes": rb, "removed": gone,
            "surviving_bytes": kept_bytes, "remove": stats(t_remove), "host_twin": stats(t_host),
            "search_behind_the_removal": stats(t_next), "fresh_add_and_first_search": stats(t_fresh),
            "memcpy_of_survivors": floor_stats(t_copy, kept_bytes), "uploads_moved": False}
    dev = [a - b for a, b in zip(t_remove, t_host)]
    line["device_by_difference"] = dict(stats(dev), estimate=True)
    floor = line["memcpy_of_survivors"]["ms"]
    line["device_over_memcpy"] = round(line["device_by_difference"]["ms"] / floor, 2) if floor else None
    line["fresh_over_remove"] = round(line["fresh_add_and_first_search"]["ms"] / line["remove"]["ms"], 2)
    line["host_twin_share_of_remove"] = round(line["host_twin"]["ms"] / line["remove"]["ms"], 3)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_mutate", "time.json"))
    a = ap.parse_args()
    _lib.load()
    if _lib.device_count() == 0:
        raise SystemExit("no GPU: nothing is measured")
    _lib.set_device(0)
    _lib.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(27)
    n = a.rows
    lines = []
    for name in ("ivfflat", "ivfpq", "ivfbin"):
        case = Case(name, n, rng)
        contiguous = np.zeros(n, bool)
        contiguous[:n // 10] = True
        masks = (("random 10 %", rng.random(n) < 0.1), ("random 50 %", rng.random(n) < 0.5), ("contiguous 10 %", contiguous),
                 ("one whole list", case.lists == 7))
        for label, m in masks:
            lines.append(removal(case, label, m, a.reps))
            print(json.dumps(lines[-1]), flush=True)
        del case
    _lib.set_stream(None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": _lib.backend(), "reps": a.reps, "lines": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
