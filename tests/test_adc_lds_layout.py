"""The LDS layout of the ADC kernels (k_adc.hip) in the built library, read from its gfx950 code objects without a GPU.

A kernel's dynamic LDS starts right after its static LDS (.group_segment_fixed_size).  The ADC kernels copy their
tables with 16-byte LDS writes and read them with 8- and 16-byte reads, which the hardware replays when the base is
off 16-byte alignment, so every ADC kernel that takes dynamic LDS must have a static size that is a multiple of 16."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vq_amd", "libvqhip.so")
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

# kernels launched with dynamic LDS, and the instantiations the schedules launch
DYNAMIC = {"k_adc_scan", "k_adc_thresh", "k_adc_scan_thr", "k_adc_sort_thr", "k_adc_sort_out"}
EXPECTED = ["k_adc_scanE", "k_adc_sort_thrE", "k_adc_sort_outE"] + [f"k_adc_threshILj{q}E" for q in (1, 2, 4, 8)] + [
    f"k_adc_scan_thrILj{q}ELj{lq}ELj512E" for q, lq in ((1, 1), (2, 1), (4, 1), (8, 2))]


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.access(path, os.X_OK) else shutil.which(name)


def _adc_kernels(tmp_path):
    """{mangled symbol: group_segment_fixed_size} of every k_adc_* kernel in the library's gfx950 code objects"""
    readelf, bundler = _tool("llvm-readelf"), _tool("clang-offload-bundler")
    if not os.path.exists(LIB):
        pytest.skip("libvqhip.so is not built")
    if not readelf or not bundler:
        pytest.skip("llvm-readelf / clang-offload-bundler not found")
    sections = subprocess.run([readelf, "-S", "-W", LIB], capture_output=True, text=True, check=True).stdout
    m = re.search(r"\.hip_fatbin\s+\S+\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)", sections)
    assert m, "no .hip_fatbin section in libvqhip.so"
    with open(LIB, "rb") as f:
        f.seek(int(m.group(1), 16))
        fatbin = f.read(int(m.group(2), 16))
    starts = [s.start() for s in re.finditer(re.escape(MAGIC), fatbin)]
    assert starts, "no offload bundles in .hip_fatbin"
    kernels = {}
    for j, s in enumerate(starts):
        bundle, co = tmp_path / f"b{j}.bin", tmp_path / f"b{j}.co"
        bundle.write_bytes(fatbin[s:starts[j + 1] if j + 1 < len(starts) else len(fatbin)])
        r = subprocess.run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}"],
                           capture_output=True, text=True)
        if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        # one .group_segment_fixed_size and one .symbol per kernel map, in that (sorted-key) order
        sizes = [int(v) for v in re.findall(r"^\s+\.group_segment_fixed_size:\s+(\d+)", notes, re.M)]
        syms = re.findall(r"^\s+\.symbol:\s+(\S+)\.kd", notes, re.M)
        assert len(sizes) == len(syms), (len(sizes), len(syms))
        for sym, size in zip(syms, sizes):
            if "k_adc_" in sym:
                kernels[sym] = size
    return kernels


def test_adc_dynamic_lds_base_is_16_byte_aligned(tmp_path):
    kernels = _adc_kernels(tmp_path)
    for want in EXPECTED:
        assert any(want in sym for sym in kernels), f"{want} not in the code objects: {sorted(kernels)}"
    bad = {}
    for sym, size in kernels.items():
        name = re.search(r"k_adc_[a-z_]+", sym).group(0)
        if name in DYNAMIC and size % 16:
            bad[sym] = size
    assert not bad, f"static LDS not a multiple of 16 in front of the dynamic tables: {bad}"
