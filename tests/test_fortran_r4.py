"""A host model built with 4-byte reals against the drop-in Fortran modules (rrtmg_lw_amd/fortran): the public names are generic over
the real kind, so tests/fortran/drive_shim_r4.f90 - drive_shim.f90 with every array real(4) - compiles against the same modules that the
real(8) host still compiles against, and its rrtmg_lw goes through rrtmg_lw_hip_run_nomcica_r4.  The compile-only part runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")
NOMCICA = ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_rad.nomcica.f90", "rrtmg_lw_adjust.f90")
MCICA = ("parkind.f90", "rrtmg_lw_init.f90", "mcica_subcol_gen_lw.f90", "rrtmg_lw_rad.f90")


def _modules(tmp, shim):
    objs = []
    for f in shim:
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    return objs


def _program(tmp, prog, objs=None):
    drv = os.path.join(tmp, prog + ".o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", prog + ".f90"), "-o", drv], check=True, cwd=tmp)
    if objs is None:
        return None
    exe, libdir = os.path.join(tmp, prog), os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}"], check=True, cwd=tmp)
    return exe


@needs_flang
def test_real4_and_real8_hosts_compile_against_the_same_modules(tmp_path):
    tmp = str(tmp_path)
    _modules(tmp, NOMCICA)
    _program(tmp, "drive_shim_r4")
    _program(tmp, "drive_shim")
    _program(tmp, "drive_adjust")
    assert os.path.exists(tmp_path / "drive_shim_r4.o") and os.path.exists(tmp_path / "drive_shim.o")


@needs_flang
def test_mcica_modules_compile_for_a_real4_host(tmp_path):
    tmp = str(tmp_path)
    _modules(tmp, MCICA)
    _program(tmp, "drive_shim_mcica_r4")
    _program(tmp, "drive_shim_mcica")
    assert os.path.exists(tmp_path / "drive_shim_mcica_r4.o")


@needs_flang
@pytest.mark.gpu
@pytest.mark.parametrize("config,icld,ndev,pin", [("cloudy", 2, 1, False), ("aer_idrv", 1, 1, False), ("cloudy", 2, 3, False), ("aer_idrv", 2, 1, True)])
def test_real4_host_model_matches_oracle(tmp_path, oracle, config, icld, ndev, pin):
    """The expected values are the oracle's on the widened float32 inputs; the bar is the real(8) shim test's 5e-5 plus the float32
    rounding of the value itself, abs(ref) * 2**-24.  ndev = 3: three virtual devices, 300 columns; pin: rrtmg_lw_pin / _static /
    _changed on real(4) arrays."""
    tmp = str(tmp_path)
    exe = _program(tmp, "drive_shim_r4", _modules(tmp, NOMCICA[:3]))
    ncol, nlay = (96, 60) if ndev == 1 else (300, 60)
    d = make_gcm_inputs(ncol, nlay, config, col0=31)
    d = {k: np.asfortranarray(v, dtype=np.float32) if isinstance(v, np.ndarray) else v for k, v in d.items()}
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([ncol, nlay, icld, d["idrv"], d["inflglw"], d["iceflglw"], d["liqflglw"]], dtype=np.int32).tofile(f)
        for k in ["play", "plev", "tlay", "tlev", "tsfc"]:
            f.write(d[k].tobytes(order="F"))
        gases = ["h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr"]
        f.write(np.stack([d[k] for k in gases], axis=2).tobytes(order="F"))
        f.write(d["emis"].tobytes(order="F"))
        f.write(np.stack([d[k] for k in ("cldfr", "cicewp", "cliqwp", "reice", "reliq")], axis=2).tobytes(order="F"))
        f.write(d["taucld"].tobytes(order="F"))
        f.write(d["tauaer"].tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    if ndev > 1:
        env.update(RRTMG_LW_NDEV=str(ndev), RRTMG_LW_VIRTUAL_DEVICES="1")
    if pin:
        env.update(DRIVE_PIN="1")
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    icld_out = int(np.frombuffer(raw, dtype=np.int32, count=1)[0])
    a = np.frombuffer(raw, dtype=np.float32, offset=4)
    wide = {k: np.asfortranarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v for k, v in d.items()}
    ref = oracle.rrtmg_lw(ncol, nlay, icld, d["idrv"], wide)
    assert icld_out == ref["icld"]
    pos = 0
    for k, nl in (("uflx", nlay + 1), ("dflx", nlay + 1), ("hr", nlay), ("uflxc", nlay + 1), ("dflxc", nlay + 1), ("hrc", nlay),
                  ("duflx_dt", nlay + 1), ("duflxc_dt", nlay + 1)):
        got = a[pos:pos + ncol * nl].reshape((ncol, nl), order="F")
        pos += ncol * nl
        if k.startswith("du") and d["idrv"] != 1:
            continue
        assert (np.abs(got.astype(np.float64) - ref[k]) <= 5e-5 + np.abs(ref[k]) * 2.0 ** -24).all(), k
