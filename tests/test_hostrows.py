"""Host logic of the host-pointer entries' row handling (rrtmg_lw_amd/csrc/hostrows.hpp): the row scan on 4- and 8-byte patterns (a float
row a,b,a,b,.. is not uniform), the widened fill value, the float64 band sum of float bands, the packing at the landing area's row stride.
The GPU side is covered by tests/test_hip_host_r4.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hostrows_scan_sum_and_packing(tmp_path):
    exe = str(tmp_path / "hostrows_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rrtmg_lw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "hostrows_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "hostrows_check: ok" in out, out
