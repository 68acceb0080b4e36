"""Adding rows to and removing rows from a resident index (include/vqhip.h, "adding and removing rows"; the compaction
of vq_amd/csrc/k_compact.hip) on one MI355X, against the two things a caller could do instead.

Two indexes: FlatIndex over 1M x 128 f32 rows (512 B a row) and BinaryIndex over 1M x 1024 bits (128 B a row).  Per index
  remove   a random 10 %, a random 50 % and the contiguous first 10 % of the rows (the mask already on the device)
  add      100k rows from device memory onto the 1M (the buffer is full: it grows and the old rows are copied), and a
           second 100k behind them (the grown buffer has room: only the new rows move)
each against
  (a) memcpy  one device-to-device copy of the bytes that survive / are appended: the floor for moving them.  The copy is
              asynchronous, so it is timed three ways side by side (the library's copy between events, the same by wall
              clock around copy + synchronise, torch's copy between events); a timing that beats the HBM peak did not
              bracket the copy: it is marked invalid and no ratio is formed from it
  (b) fresh   what there was before: a new index created from the host rows that remain (the upload included)
Device forms, HIP events on the stream the library launches on (the calls return synchronised, so the events bracket all
of a call), the legs of one line alternated in one process, the median of --reps with its extremes.  A removal changes the
index, so every repetition of one starts from an index created again from the rows on the device (not timed).

    python tools/mutate_time.py [--reps 5] [--rows 1000000] [--out profiles/mutate/time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vq_amd import _lib  # noqa: E402


def stats(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def timed(fn):
    """milliseconds of fn() between two events on the current stream (the library's, through set_stream)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    _lib.synchronize()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


HBM_PEAK_GBPS = 8000.0  # MI355X: nothing that reads and writes `moved` bytes of HBM finishes faster than this


def copy_floor(dst, src, nbytes, reps_ms):
    """The floor (a), a device-to-device copy of `nbytes`, timed three ways in one repetition: the library's copy between
    events, the same with a wall clock around copy + synchronise, and torch's own copy of the same bytes between events.
    An asynchronous call is only as well timed as its events bracket it, so the three are kept side by side."""
    reps_ms["events"].append(timed(lambda: _lib.memcpy_device(dst.data_ptr(), src.data_ptr(), nbytes)))
    reps_ms["wall"].append(wall(lambda: _lib.memcpy_device(dst.data_ptr(), src.data_ptr(), nbytes)))
    flat_src = src.view(torch.uint8).reshape(-1)[:nbytes]
    reps_ms["torch_events"].append(timed(lambda: dst[:nbytes].copy_(flat_src)))


def floor_stats(reps_ms, nbytes):
    """The three timings with their rates (read + written bytes).  `ms`, the floor ratios are formed from, is torch's copy
    between events, and only where it is believable: not faster than the HBM peak, and not faster than half of what the
    wall clock saw around the library's copy and its synchronise (which can only be too slow, by the launch and the
    wait).  None otherwise.  The library's own copy between events is recorded but never used: on the MI355X it reads
    about 6 us at every size (151 TB/s for 461 MB), so those events do not bracket the copy -- and for a small copy such a
    figure stays under the peak, so that the peak alone cannot tell."""
    out = {}
    for k, v in reps_ms.items():
        s = stats(v)
        s["gbps"] = round(2 * nbytes / s["ms"] / 1e6, 1) if s["ms"] > 0 else None
        s["below_hbm_peak"] = s["gbps"] is not None and s["gbps"] <= HBM_PEAK_GBPS
        out[k] = s
    t, w = out["torch_events"], out["wall"]
    ok = t["below_hbm_peak"] and w["below_hbm_peak"] and t["ms"] >= 0.5 * w["ms"] - 0.02  # (0.02 ms: a launch and a wait)
    out["events"]["used"] = False
    out["ms"] = t["ms"] if ok else None
    if not ok:
        out["no_floor_because"] = "torch's copy between events and the wall clock around the library's copy disagree, or one beats the HBM peak"
    return out


def checked(line, key, moved):
    """an event-timed leg of the feature itself: its rate, and the same validity mark"""
    g = round(moved / line[key]["ms"] / 1e6, 1)
    line[key]["gbps"] = g
    line[key]["valid"] = g <= HBM_PEAK_GBPS
    return line[key]["valid"]


class Case:
    """one index kind: how a handle is made from device rows and from host rows, and its row width"""

    def __init__(self, name, n, rng):
        self.name, self.n = name, n
        if name == "flat":
            self.d, self.rb = 128, 512
            self.host = rng.standard_normal((n, 128)).astype(np.float32)
        else:
            self.d, self.rb = 1024, 128
            self.host = rng.integers(0, 1 << 32, (n, 32), dtype=np.uint64).astype(np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.int32)).to("cuda")
        torch.cuda.synchronize()

    def from_device(self, ptr, n):
        if self.name == "flat":
            return _lib.Flat(self.host[:1], _lib.EUCLIDEAN, dev_rows=ptr, shape=(n, self.d))
        return _lib.Binary(None, _lib.BINARY_PACKED, n, self.d, 0.0, 0, 1, _lib.MANHATTAN, dev_src=ptr)

    def from_host(self, rows):
        if self.name == "flat":
            return _lib.Flat(rows, _lib.EUCLIDEAN)
        return _lib.Binary(rows, _lib.BINARY_PACKED, rows.shape[0], self.d, 0.0, 0, 1, _lib.MANHATTAN)

    def add(self, h, ptr, b):
        if self.name == "flat":
            h.add("add_device", ptr, b)
        else:
            h.add("add_device", ptr, b, _lib.BINARY_PACKED)


def removal(case, name, m, reps):
    n, rb = case.n, case.rb
    words = np.packbits(m, bitorder="little")
    words = np.concatenate([words, np.zeros((-len(words)) % 4, np.uint8)]).view(np.uint32)
    w = torch.from_numpy(words.view(np.int32).copy()).to("cuda")
    kept_bytes = int((~m).sum()) * rb
    scratch = torch.empty(kept_bytes, dtype=torch.uint8, device="cuda")
    survivors = np.ascontiguousarray(case.host[~m])
    torch.cuda.synchronize()
    t_remove, t_fresh = [], []
    t_copy = {"events": [], "wall": [], "torch_events": []}
    for _ in range(reps):
        h = case.from_device(case.dev.data_ptr(), n)
        t_remove.append(timed(lambda: h.remove(w.data_ptr())))
        assert h.n == n - int(m.sum())
        h.close()
        copy_floor(scratch, case.dev, kept_bytes, t_copy)
        f = [None]
        t_fresh.append(wall(lambda: f.__setitem__(0, case.from_host(survivors))))
        f[0].close()
    line = {"index": case.name, "op": "remove", "mask": name, "n": n, "row_bytes": rb, "removed": int(m.sum()),
            "surviving_bytes": kept_bytes, "remove": stats(t_remove), "memcpy_of_survivors": floor_stats(t_copy, kept_bytes),
            "fresh_index_from_host": stats(t_fresh)}
    # the removal reads every mask word and the surviving rows and writes them: 2 x the surviving bytes at the least
    ok = checked(line, "remove", 2 * kept_bytes)
    floor = line["memcpy_of_survivors"]["ms"]
    line["remove_over_memcpy"] = round(line["remove"]["ms"] / floor, 3) if ok and floor else None
    line["fresh_over_remove"] = round(line["fresh_index_from_host"]["ms"] / line["remove"]["ms"], 2) if ok else None
    return line


def addition(case, b, reps):
    n, rb = case.n, case.rb
    extra = case.dev[:b].clone()
    scratch = torch.empty(b * rb, dtype=torch.uint8, device="cuda")
    both = np.ascontiguousarray(np.concatenate([case.host, case.host[:b]]))
    torch.cuda.synchronize()
    t_grow, t_room, t_fresh = [], [], []
    t_copy = {"events": [], "wall": [], "torch_events": []}
    for _ in range(reps):
        h = case.from_device(case.dev.data_ptr(), n)
        t_grow.append(timed(lambda: case.add(h, extra.data_ptr(), b)))
        t_room.append(timed(lambda: case.add(h, extra.data_ptr(), b)))
        assert h.n == n + 2 * b
        h.close()
        copy_floor(scratch, extra, b * rb, t_copy)
        f = [None]
        t_fresh.append(wall(lambda: f.__setitem__(0, case.from_host(both))))
        f[0].close()
    line = {"index": case.name, "op": "add", "n": n, "row_bytes": rb, "added": b, "added_bytes": b * rb,
            "add_that_grows": stats(t_grow), "add_with_room": stats(t_room), "memcpy_of_added": floor_stats(t_copy, b * rb),
            "fresh_index_from_host": stats(t_fresh), "grow_copies_bytes": n * rb}
    ok_g = checked(line, "add_that_grows", 2 * (n + b) * rb)  # the old rows and the new ones, read and written
    ok_r = checked(line, "add_with_room", 2 * b * rb)
    floor = line["memcpy_of_added"]["ms"]
    line["fresh_over_add_that_grows"] = round(line["fresh_index_from_host"]["ms"] / line["add_that_grows"]["ms"], 2) if ok_g else None
    line["add_with_room_over_memcpy"] = round(line["add_with_room"]["ms"] / floor, 3) if ok_r and floor else None
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mutate", "time.json"))
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    _lib.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(26)
    n = a.rows
    lines = []
    for name in ("flat", "binary"):
        case = Case(name, n, rng)
        contiguous = np.zeros(n, bool)
        contiguous[:n // 10] = True
        for label, m in (("random 10 %", rng.random(n) < 0.1), ("random 50 %", rng.random(n) < 0.5), ("contiguous 10 %", contiguous)):
            lines.append(removal(case, label, m, a.reps))
            print(json.dumps(lines[-1]), flush=True)
        lines.append(addition(case, n // 10, a.reps))
        print(json.dumps(lines[-1]), flush=True)
        del case
    _lib.set_stream(None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": _lib.backend(), "reps": a.reps, "lines": lines}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
