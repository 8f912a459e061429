"""The ownership types of the driver's GPU resources (rrtmg_lw_amd/csrc/owned.hpp) over counting traits: every acquire and release is
recorded with its handle - construction, moves, reset, the create-into-slot accessor, GrowBuf::reserve below / at / above the capacity and
with a failing acquire or release, the never-destroyed storage of the globals.  Built plain and with AddressSanitizer + UBSan (a handle is
a heap object: a second release is a double free, a forgotten one a leak; the sanitizers' runtimes are linked into the program, so that it
runs whatever else the environment loads into a process).  The GPU side is covered by tests/test_hip_lifecycle.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                    "-static-libasan", "-static-libubsan")],
                         ids=["plain", "sanitized"])
def test_owned_types_release_exactly_once(tmp_path, flags):
    exe = str(tmp_path / "owned_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", os.path.join(ROOT, "rrtmg_lw_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "owned_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "owned_check: ok" in out, out
