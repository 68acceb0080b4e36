"""Once-only exhaustive check: every one of the 2^32 f32 bit patterns through the device encoder, against the numpy
restatement of the reference (tests/ref_sqbq.py), for ScalarQuantizer(-1, 1, 256) and BinaryQuantizer(0, 0, 1).
Prints (and with --out writes) one JSON object with the mismatch counts; minutes on one MI355X, most of them numpy.

    python tools/sqbq_exhaustive.py [--out profiles/sqbq_exhaustive.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_sqbq as R  # noqa: E402
import vq_amd  # noqa: E402
from vq_amd import _lib  # noqa: E402

CHUNK = 1 << 26


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    cases = {"sq(-1,1,256)": (vq_amd.ScalarQuantizer(-1.0, 1.0, 256), lambda x: R.sq_encode(-1.0, 1.0, 256, x)),
             "bq(0,0,1)": (vq_amd.BinaryQuantizer(0.0, 0, 1), lambda x: R.bq_encode(0.0, 0, 1, x))}
    res = {"patterns": 1 << 32, "backend": _lib.backend()}
    dx = torch.empty(CHUNK, dtype=torch.float32, device="cuda")
    dc = torch.empty(CHUNK, dtype=torch.uint8, device="cuda")
    pool = ThreadPoolExecutor(8)
    t0 = time.time()
    for name, (q, ref) in cases.items():
        bad, first = 0, None
        for base in range(0, 1 << 32, CHUNK):
            bits = np.arange(base, base + CHUNK, dtype=np.uint64).astype(np.uint32)
            x = bits.view(np.float32)
            dx.copy_(torch.from_numpy(x))
            torch.cuda.synchronize()
            q.quantize_device(dx.data_ptr(), CHUNK, dc.data_ptr())
            _lib.synchronize()
            got = dc.cpu().numpy()
            parts = np.array_split(np.arange(CHUNK), 8)
            want = np.concatenate(list(pool.map(lambda p: ref(x[p[0]:p[-1] + 1]), parts)))
            miss = np.flatnonzero(got != want)
            if miss.size and first is None:
                first = {"bits": f"{int(bits[miss[0]]):#010x}", "got": int(got[miss[0]]), "want": int(want[miss[0]])}
            bad += int(miss.size)
        res[name] = {"mismatches": bad, "first": first}
    res["seconds"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(res[k]["mismatches"] == 0 for k in cases) else 1


if __name__ == "__main__":
    sys.exit(main())
