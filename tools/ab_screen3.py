"""A/B of two library builds on the sub_dim-16 encode screen by row family (C2's shape: 1M x 128, m = 8, k = 256): uniform,
N(0,1) and clustered rows -- encode time, the screen and re-check stages (HIP events), the re-checked fraction, the number
of bf16 products of the screen that ran (0 on a build without the export) and a crc of the codes.  A family named
`kind:sd` runs at that sub_dim instead (1M x 8 sd; `uniform:14`, `uniform:15`: the padded forms of the same screen).
    VQHIP_LIB_PATH=ab/libvqhip_base.so python tools/ab_screen3.py ; python tools/ab_screen3.py    (alternate a few times)"""
import os, sys, time, zlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vq_amd import _lib
_lib.load(); _lib.set_device(0)
tag = os.path.basename(os.environ.get("VQHIP_LIB_PATH", "new"))
n, m, k = 1_000_000, 8, 256


def rows(kind, d):
    g = torch.Generator(device="cuda").manual_seed(66)
    if kind == "uniform":
        return torch.rand((n, d), generator=g, device="cuda")
    if kind == "normal":
        return torch.randn((n, d), generator=g, device="cuda")
    centers = torch.randn((40, d), generator=g, device="cuda") * 3  # tests/test_gpu_piped.py's clustered family
    pick = torch.randint(0, 40, (n,), generator=g, device="cuda")
    return centers[pick] + 0.05 * torch.randn((n, d), generator=g, device="cuda")


def run(name, reps=6, inner=25):
    kind, _, sd = name.partition(":")
    d = m * int(sd or 16)
    X = rows(kind, d).contiguous()
    torch.cuda.synchronize()
    ds = _lib.Dataset.from_device(X.data_ptr(), n, d, keepalive=X)
    km = _lib.KMeans(ds, m, k)
    km.init_from_rows(np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64))
    for _ in range(2): km.step()
    enc = _lib.PQEncoder(km.get_centroids(), 0)
    dcodes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    for _ in range(8 * inner): enc.encode_device(ds.device_ptr, n, dcodes.data_ptr(), None)  # clocks up
    _lib.synchronize()
    te = []
    for _ in range(reps):
        _lib.synchronize(); t0 = time.perf_counter()
        for _ in range(inner): enc.encode_device(ds.device_ptr, n, dcodes.data_ptr(), None)
        _lib.synchronize(); te.append((time.perf_counter() - t0) / inner * 1e3)
    rech, eng = _lib.last_assign_stats()
    prod = _lib.last_screen_products() if hasattr(_lib.load(), "vqhip_last_screen_products") else 0
    _lib.set_profiling(True)
    for _ in range(inner): enc.encode_device(ds.device_ptr, n, dcodes.data_ptr(), None)
    calls, ms_screen, ms_recheck = _lib.profile_collect()
    _lib.set_profiling(False)
    crc = zlib.crc32(np.ascontiguousarray(dcodes.cpu().numpy()).tobytes()) & 0xffffffff
    te_s = sorted(te)
    print(f"{tag:20s} {name:9s}: encode ms min {min(te):.4f} median {te_s[len(te_s) // 2]:.4f}  screen {ms_screen / calls:.4f} recheck {ms_recheck / calls:.4f}"
          f"  rechecked {rech} ({100.0 * rech / (n * m):.3f} %) products {prod} crc {crc:08x}", flush=True)
    enc.close(); km.close(); ds.close()


for name in (sys.argv[1:] or ["uniform", "normal", "clustered", "uniform:14", "uniform:15"]):
    run(name)
