"""rrtmg_lw_cloud_optics (module rrtmg_lw_optics) and rrtmg_lw_cloud_optics_dev (module rrtmg_lw_device) from a flang-built host model
(tests/fortran/drive_cloud_optics.f90), built as tests/test_fortran_cloud_cover.py builds its drivers: the host routine on arrays
larger than the call (pcols > ncol), the device routine on columns inside wider device fields; what comes back equals the C entry's
numbers (the Python host entry) bit for bit, and nothing outside the call's columns is written.  The compile-only part runs without a
GPU."""
import os
import subprocess

import numpy as np
import pytest

import cloud_states as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")
NCOL = 45
IN = ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq", "plev", "h2ovmr")


def _compile(tmp, link=True):
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_optics.f90", "rrtmg_lw_device.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_cloud_optics.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_cloud_optics.f90"), "-o", drv], check=True, cwd=tmp)
    if not link:
        return None
    exe = os.path.join(tmp, "drive_cloud_optics")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, cwd=tmp)
    return exe


@needs_flang
def test_modules_and_driver_compile(tmp_path):
    _compile(str(tmp_path), link=False)
    assert os.path.exists(tmp_path / "rrtmg_lw_optics.mod") and os.path.exists(tmp_path / "rrtmg_lw_device.mod")


@needs_flang
@pytest.mark.gpu
def test_host_and_device_routines_equal_the_c_entry(tmp_path, hip):
    tmp = str(tmp_path)
    exe = _compile(tmp)
    d = cs.take(cs.family_b()[(2, 1, 1)], slice(30, 30 + NCOL))
    nlay = d["nlay"]
    for imca in (0, 1):
        want = hip.cloud_optics(d, imca=imca)
        assert want["taucloud"].any() and len(set(want["ncbands"])) > 1 - imca
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            np.array([NCOL, nlay, imca, d["inflglw"], d["iceflglw"], d["liqflglw"]], dtype=np.int32).tofile(f)
            for k in IN:
                f.write(np.asfortranarray(d[k], dtype=np.float64).tobytes(order="F"))
        env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
                   RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
        assert np.frombuffer(raw, dtype=np.int32, count=1)[0] == 0, "elements outside the call's columns were written, or the lone output differs"
        at = 8
        for who in ("host", "device"):
            tau = np.frombuffer(raw, dtype=np.float64, offset=at, count=NCOL * nlay * 16).reshape((NCOL, nlay, 16), order="F")
            at += tau.nbytes
            sec = np.frombuffer(raw, dtype=np.float64, offset=at, count=NCOL * 16).reshape((NCOL, 16), order="F")
            at += sec.nbytes
            nb = np.frombuffer(raw, dtype=np.int32, offset=at, count=NCOL)
            at += nb.nbytes
            assert np.array_equal(tau, want["taucloud"]), (who, imca)
            assert np.array_equal(sec, want["secdiff"]), (who, imca)
            assert np.array_equal(nb, want["ncbands"]), (who, imca)
        assert at == len(raw)
