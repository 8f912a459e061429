"""The Fortran module rrtmg_lw_optics (rrtmg_lw_amd/fortran/rrtmg_lw_optics.f90): it compiles (no GPU), and a flang host model that calls
rrtmg_lw_gas_optics with and without the optional Planck outputs gets what api.gas_optics returns, bit for bit
(tests/fortran/drive_optics.f90)."""
import os
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
GASES = ("h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")


def _build(tmp):
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_optics.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_optics.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_optics.f90"), "-o", drv], check=True, cwd=tmp)
    return objs, drv


@needs_flang
def test_optics_module_compiles(tmp_path):
    objs, _ = _build(str(tmp_path))
    syms = subprocess.run(["nm", objs[-1]], capture_output=True, text=True).stdout
    assert "rrtmg_lw_hip_gas_optics" in syms


@needs_flang
@pytest.mark.gpu
def test_fortran_host_model_optics_matches_python(tmp_path, hip):
    tmp = str(tmp_path)
    objs, drv = _build(tmp)
    exe = os.path.join(tmp, "drive_optics")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}"], check=True, cwd=tmp)
    ncol, nlay, ng = 96, 60, hip.gpoints()
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=31)
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([ncol, nlay, ng], dtype=np.int32).tofile(f)
        for k in ("play", "plev", "tlay", "tlev", "tsfc"):
            f.write(np.asfortranarray(d[k]).tobytes(order="F"))
        f.write(np.stack([d[k] for k in GASES], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(d["emis"]).tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    a = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
    want = hip.gas_optics(d, idrv=1)
    plain = hip.gas_optics(d, idrv=0, out=dict(planklay=None, planklev=None, plankbnd=None))
    shapes = (("taug", (ncol, nlay, ng)), ("fracs", (ncol, nlay, ng)), ("planklay", (ncol, nlay, 16)), ("planklev", (ncol, nlay + 1, 16)),
              ("plankbnd", (ncol, 16)), ("dplankbnd_dt", (ncol, 16)), ("taug2", (ncol, nlay, ng)), ("fracs2", (ncol, nlay, ng)))
    pos = 0
    for k, shape in shapes:
        n = int(np.prod(shape))
        got = a[pos:pos + n].reshape(shape, order="F")
        pos += n
        ref = plain[k[:-1]] if k.endswith("2") else want[k]
        assert np.array_equal(got, ref), k
    assert pos == a.size
