"""ScalarQuantizer / BinaryQuantizer rates on one MI355X; prints one JSON line.

Device forms at 1M x 384 (HIP-event ms per call, median of --reps; effective TB/s = bytes read + bytes written per call:
5 bytes per element either way), the host form (host array in, host codes out, caller's `out=`), and the per-vector
call latency at d = 384 (median wall time of `quantize` / `dequantize`).

    python tools/sqbq_time.py [--reps 50]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from vq_amd import _lib  # noqa: E402


def event_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        fn()
        b.record(torch.cuda.current_stream())
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=384)
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    torch.cuda.set_device(0)
    # the library's launches on the stream the events time: a stream of its own (the default stream's handle is 0,
    # which would hand the library back its own per-thread stream)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    _lib.set_stream(stream.cuda_stream)
    n, d = a.n, a.d
    count = n * d
    x = torch.rand((n, d), device="cuda") * 2.2 - 1.1
    codes = torch.randint(0, 256, (n, d), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sq, bq = vq_amd.ScalarQuantizer(-1.0, 1.0, 256), vq_amd.BinaryQuantizer(0.0)
    sq_inf = vq_amd.ScalarQuantizer(-3e38, 3e38, 256)  # step = inf: the direct kernel
    nbytes = 5 * count
    res = {"n": n, "d": d}
    kernels = {
        "sq_encode": lambda: sq.quantize_device(x.data_ptr(), count, codes.data_ptr()),
        "sq_encode_direct_inf_step": lambda: sq_inf.quantize_device(x.data_ptr(), count, codes.data_ptr()),
        "sq_decode": lambda: sq.dequantize_device(codes.data_ptr(), count, out.data_ptr()),
        "bq_encode": lambda: bq.quantize_device(x.data_ptr(), count, codes.data_ptr()),
        "bq_decode": lambda: bq.dequantize_device(codes.data_ptr(), count, out.data_ptr()),
        "copy_f32_to_f32_ref": lambda: out.copy_(x),  # torch's copy of the same 1.5 GB: 8 bytes per element
    }
    for name, fn in kernels.items():
        ms = event_ms(fn, a.reps)
        b = 8 * count if name.startswith("copy") else nbytes
        res[name] = {"ms": round(ms, 4), "TBps": round(b / ms / 1e9, 3)}
    _lib.set_stream(None)
    # host form: host rows in, host codes out (PCIe-bound)
    xh = x.cpu().numpy()
    ch = np.empty((n, d), np.uint8)
    oh = np.empty((n, d), np.float32)
    for name, fn in (("sq_encode_host", lambda: sq.quantize_batch(xh, out=ch)),
                     ("sq_decode_host", lambda: sq.dequantize_batch(ch, out=oh))):
        fn()
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        s = float(np.median(t))
        res[name] = {"ms": round(s * 1e3, 2), "GBps": round(nbytes / s / 1e9, 2), "elements_per_s": round(count / s, 0)}
    # per-vector latency at d = 384
    v = xh[0].copy()
    c = sq.quantize(v)
    for name, fn in (("sq_quantize_1x384", lambda: sq.quantize(v)), ("sq_dequantize_1x384", lambda: sq.dequantize(c)),
                     ("bq_quantize_1x384", lambda: bq.quantize(v))):
        for _ in range(50):
            fn()
        t = []
        for _ in range(2000):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        res[name] = {"us_median": round(float(np.median(t)) * 1e6, 1), "us_p90": round(float(np.percentile(t, 90)) * 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
