"""What the event markers of an encode step cost: one encoder, four settings alternated inside ONE process.

    python tools/step_markers_time.py [--out profiles/step_markers/NAME.json]
    VQHIP_LIB_PATH=other/libvqhip.so python tools/step_markers_time.py      (another build of the library)

The settings are {library-owned stream, caller-set stream (vqhip_set_stream)} x {profiling hooks off, on}.  A step
is one `encode_device` pass; the shapes are C2 (1M x 128, m = 8, k = 256: two kernels of 0.23 + 0.02 ms) and C1
(10k x 64, m = 4, k = 16: one kernel of a few microseconds).  Rows come from `Dataset.synthetic`, codebooks from 4
Lloyd iterations; 300 untimed passes bring the clocks up, then every setting is timed 5 times over 20 passes, the
settings taking turns, and the median of the 5 is reported.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vq_amd import _lib

SETTINGS = [("library_stream_hooks_off", False, False), ("library_stream_hooks_on", False, True),
            ("caller_stream_hooks_off", True, False), ("caller_stream_hooks_on", True, True)]


def shape(label, n, d, m, k, stream, rounds=5, inner=20, untimed=300):
    ds = _lib.Dataset.synthetic(n, d, 66, 0)
    km = _lib.KMeans(ds, m, k)
    km.init_from_rows(np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64))
    for _ in range(4):
        km.step()
    enc = _lib.PQEncoder(km.get_centroids(), 0)
    codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def passes(count):
        for _ in range(count):
            enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)

    def select(own_stream, hooks):
        _lib.synchronize()
        _lib.set_stream(stream.cuda_stream if own_stream else None)
        _lib.set_profiling(hooks)
        passes(1)  # the handle's order behind the other stream is paid here, not in the timed passes
        _lib.synchronize()

    _lib.set_stream(None)
    passes(untimed)
    _lib.synchronize()
    times = {name: [] for name, _, _ in SETTINGS}
    stages = {}
    for _ in range(rounds):
        for name, own_stream, hooks in SETTINGS:
            select(own_stream, hooks)
            if hooks:
                _lib.profile_collect()
            t0 = time.perf_counter()
            passes(inner)
            _lib.synchronize()
            times[name].append((time.perf_counter() - t0) / inner * 1e3)
            if hooks:
                calls, primary_ms, recheck_ms = _lib.profile_collect()
                stages.setdefault(name, []).append([primary_ms / max(1, calls), recheck_ms / max(1, calls)])
    _lib.set_profiling(False)
    _lib.set_stream(None)
    rechecked, engine = _lib.last_assign_stats()
    out = {"shape": label, "rows": n, "dim": d, "m": m, "k": k, "engine": int(engine), "rechecked": int(rechecked),
           "passes_per_timing": inner, "timings_per_setting": rounds,
           "ms_per_step_median": {name: float(np.median(v)) for name, v in times.items()},
           "ms_per_step_all": {name: [round(x, 5) for x in v] for name, v in times.items()},
           "stage_ms_per_step_median": {name: [float(np.median([r[0] for r in v])), float(np.median([r[1] for r in v]))]
                                        for name, v in stages.items()}}
    base = out["ms_per_step_median"]["library_stream_hooks_off"]
    out["ms_over_library_stream_hooks_off"] = {name: v - base for name, v in out["ms_per_step_median"].items()}
    enc.close()
    km.close()
    ds.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    stream = torch.cuda.Stream()
    result = {"tool": "step_markers_time", "library": os.environ.get("VQHIP_LIB_PATH", "vq_amd/libvqhip.so"),
              "shapes": [shape("C2", 1_000_000, 128, 8, 256, stream), shape("C1", 10_000, 64, 4, 16, stream)]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
