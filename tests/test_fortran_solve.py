"""rrtmg_lw_solve (module rrtmg_lw_optics) from a flang-built host model (tests/fortran/drive_solve.f90), built as
tests/test_fortran_cloud_optics.py builds its driver: the host routine on arrays larger than the call (pcols > ncol) returns the C
entry's numbers (the Python host entry) bit for bit, and nothing outside the call's columns is written.  The compile-only part runs
without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")
NCOL, NLAY = 70, 5
IN = ("plev", "emis", "tau", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt", "cldfr", "odcld", "submask")
LEVELS = ("uflx", "dflx", "uflxc", "dflxc", "duflx_dt", "duflxc_dt")


def _compile(tmp, link=True):
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_optics.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_solve.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_solve.f90"), "-o", drv], check=True, cwd=tmp)
    if not link:
        return None
    exe = os.path.join(tmp, "drive_solve")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, cwd=tmp)
    return exe


@needs_flang
def test_module_and_driver_compile(tmp_path):
    _compile(str(tmp_path), link=False)
    assert os.path.exists(tmp_path / "rrtmg_lw_optics.mod") and os.path.exists(tmp_path / "drive_solve.o")


@needs_flang
@pytest.mark.gpu
def test_host_routine_equals_the_c_entry(tmp_path, hip):
    tmp = str(tmp_path)
    exe = _compile(tmp)
    d = sr.designed_inputs(NCOL, NLAY, 140)
    for cloud, idrv in ((0, 0), (1, 1), (2, 1)):
        want = hip.solve(dict(d), cloud=cloud, idrv=idrv)
        assert want["uflx"].all() and (cloud == 0 or (want["uflx"] != want["uflxc"]).any())
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            np.array([NCOL, NLAY, cloud, idrv, 140, 5], dtype=np.int32).tofile(f)
            for k in IN:
                f.write(np.asfortranarray(d[k]).tobytes(order="F"))
        env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
                   RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
        assert np.frombuffer(raw, dtype=np.int32, count=1)[0] == 0, "elements outside the call's columns were written, or the exactly sized call differs"
        at = 8
        for k in LEVELS + ("hr", "hrc"):
            n = NLAY if k.startswith("hr") else NLAY + 1
            a = np.frombuffer(raw, dtype=np.float64, offset=at, count=NCOL * n).reshape((NCOL, n), order="F")
            at += a.nbytes
            if k.startswith("du") and idrv == 0:
                continue
            assert np.array_equal(a, want[k]), (k, cloud, idrv)
        assert at == len(raw)
