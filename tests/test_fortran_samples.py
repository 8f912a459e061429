"""Module rrtmg_lw_samples (rrtmg_lw_amd/fortran/rrtmg_lw_samples.f90) compiled with flang into a small host model
(tests/fortran/drive_samples.f90), built as tests/test_fortran_shim.py builds its drivers: the mean over three samples of 70 columns
equals the Python host entry's bit for bit.  The compile-only part runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")
GASES = ("h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr")


def _compile(tmp, link):
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_samples.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_samples.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_samples.f90"), "-o", drv], check=True, cwd=tmp)
    if not link:
        return None
    exe = os.path.join(tmp, "drive_samples")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}"], check=True, cwd=tmp)
    return exe


@needs_flang
def test_samples_module_compiles(tmp_path):
    _compile(str(tmp_path), link=False)
    assert os.path.exists(tmp_path / "rrtmg_lw_samples.mod")


@needs_flang
@pytest.mark.gpu
def test_fortran_host_model_equals_python_host_entry(tmp_path, hip, oracle):
    tmp = str(tmp_path)
    exe = _compile(tmp, link=True)
    ncol, nlay, icld, seed, nsamp, step = 70, 40, 2, 280, 3, 140
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=31)
    alpha = np.zeros((ncol, nlay))
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([ncol, nlay, icld, d["idrv"], d["inflglw"], d["iceflglw"], d["liqflglw"], seed, nsamp, step, 0], dtype=np.int32).tofile(f)
        for k in ("play", "plev", "tlay", "tlev", "tsfc"):
            f.write(np.asfortranarray(d[k]).tobytes(order="F"))
        f.write(np.stack([d[k] for k in GASES], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(d["emis"]).tobytes(order="F"))
        f.write(np.stack([d[k] for k in ("cldfr", "cicewp", "cliqwp", "reice", "reliq")], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(alpha).tobytes(order="F"))
        f.write(np.asfortranarray(d["taucld"]).tobytes(order="F"))
        f.write(np.asfortranarray(d["tauaer"]).tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    icld_out = int(np.frombuffer(raw, dtype=np.int32, count=1)[0])
    a = np.frombuffer(raw, dtype=np.float64, offset=4)
    want = hip.rrtmg_lw_mcica_subcol_from_dict(d, seed, 0, alpha=alpha, icld=icld, nsamp=nsamp, seedstep=step)
    assert icld_out == want["icld"]
    pos = 0
    for k, nl in (("uflx", nlay + 1), ("dflx", nlay + 1), ("hr", nlay), ("uflxc", nlay + 1), ("dflxc", nlay + 1), ("hrc", nlay)):
        got = a[pos:pos + ncol * nl].reshape((ncol, nl), order="F")
        pos += ncol * nl
        assert np.array_equal(got, want[k]), k
    single = hip.rrtmg_lw_mcica_subcol_from_dict(d, seed, 0, alpha=alpha, icld=icld)
    assert np.abs(single["uflx"] - want["uflx"]).max() > 0.1          # (a mean, not sample 0)
