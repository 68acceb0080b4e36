"""Driver of tests/cpp/test_adc_plan.cpp: the ADC search's LDS plan (vq_amd/csrc/adc_plan.hpp) builds with g++ alone and
keeps both schedules inside the CU's 160 KiB for every table they take."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_adc_lds_plan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = tmp_path / "test_adc_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "vq_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_adc_plan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PLAN_OK" in r.stdout, r.stdout + r.stderr
