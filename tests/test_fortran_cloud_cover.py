"""rrtmg_lw_cloud_cover (module rrtmg_lw_cover, rrtmg_lw_amd/fortran/rrtmg_lw_cover.f90) and rrtmg_lw_cloud_cover_dev (module
rrtmg_lw_device) from flang-built host models (tests/fortran/drive_cloud_cover.f90, drive_cloud_cover_dev.f90), built as
tests/test_fortran_shim.py builds its drivers: both real kinds, one sample with the packed mask and three samples without; what comes
back equals the Python entry's output bit for bit.  The compile-only part runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import cloud_cover_ref as ccr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")
NCOL, NLAY, SEED, MW = 70, 13, 421, 5


def _compile(tmp, wp, device, link=True):
    module = "rrtmg_lw_device.f90" if device else "rrtmg_lw_cover.f90"
    name = "drive_cloud_cover_dev" if device else "drive_cloud_cover"
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", module):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, name + ".o")
    subprocess.run([FLANG, "-cpp", f"-DWP={wp}", "-c", "-O2", os.path.join(ROOT, "tests", "fortran", name + ".f90"), "-o", drv], check=True, cwd=tmp)
    if not link:
        return None
    exe = os.path.join(tmp, name)
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    hiplib = ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"] if device else []
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}", *hiplib], check=True, cwd=tmp)
    return exe


@needs_flang
@pytest.mark.parametrize("wp", [8, 4])
def test_modules_and_drivers_compile(tmp_path, wp):
    _compile(str(tmp_path), wp, device=False, link=False)
    assert os.path.exists(tmp_path / "rrtmg_lw_cover.mod")
    _compile(str(tmp_path), wp, device=True, link=False)


def _inputs(oracle, icld, wp):
    """the designed fields, as a host of that real kind holds them and widened again; alpha from the oracle, rounded likewise"""
    g = ccr.designed_inputs(NCOL, NLAY, seed=9)
    dt = np.float64 if wp == 8 else np.float32
    rnd = lambda a: np.asfortranarray(np.asarray(a).astype(dt).astype(np.float64))
    play, cldfr = rnd(g["play"]), rnd(g["cldfr"])
    alpha = np.zeros((NCOL, NLAY), order="F")
    if icld in (4, 5):
        alpha = rnd(oracle.get_alpha(NCOL, NLAY, icld, 0, 2500.0, g["dz"], g["lat"], 100, cldfr))
    return play, cldfr, alpha


def _drive(tmp, exe, icld, nsamp, step, irng, play, cldfr, alpha, device):
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([NCOL, NLAY, icld, SEED, nsamp, step, irng], dtype=np.int32).tofile(f)
        for a in (play, cldfr, alpha):
            f.write(np.asfortranarray(a).tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    head = np.frombuffer(raw, dtype=np.int32, count=2)
    nf = NCOL + 2 * NCOL * NLAY + (0 if device else NCOL)
    a = np.frombuffer(raw, dtype=np.float64, offset=8, count=nf)
    out = {"cldtot": a[:NCOL], "cldcum": a[NCOL:NCOL + NCOL * NLAY].reshape((NCOL, NLAY), order="F"),
           "cldlay": a[NCOL + NCOL * NLAY:NCOL + 2 * NCOL * NLAY].reshape((NCOL, NLAY), order="F")}
    if not device:
        out["tot2"] = a[NCOL + 2 * NCOL * NLAY:]
    out["submask"] = np.frombuffer(raw, dtype=np.uint32, offset=8 + 8 * nf).reshape((NCOL, NLAY, MW), order="F")
    return head, out


def _check(hip, head, got, icld, nsamp, step, irng, play, cldfr, alpha, wp):
    """against the Python host entry on the widened inputs (float32: its float64 results rounded once)"""
    dt = np.float64 if wp == 8 else np.float32
    names = ("cldtot", "cldcum", "cldlay") + (("submask",) if nsamp == 1 else ())
    want = hip.mcica_cloud_cover(NCOL, NLAY, icld, SEED, irng, play, cldfr, alpha=alpha if icld in (4, 5) else None, nsamp=nsamp, seedstep=step,
                                 outputs=names)
    assert head[0] == want["irng"]
    for k in names[:3]:
        assert np.array_equal(got[k], want[k].astype(dt).astype(np.float64)), k
    assert ((want["cldtot"] > 0) & (want["cldtot"] < 1)).any()
    if nsamp == 1:
        assert np.array_equal(got["submask"], want["submask"])
    else:
        assert (got["submask"] == 0xFFFFFFFF).all()            # (not passed: not touched)
    return want


@needs_flang
@pytest.mark.gpu
@pytest.mark.parametrize("wp", [8, 4])
def test_host_generic_equals_the_python_entry(tmp_path, hip, oracle, wp):
    tmp = str(tmp_path)
    exe = _compile(tmp, wp, device=False)
    for icld, nsamp, step, irng in ((2, 1, 140, 0), (5, 3, 140, 0), (4, 1, 140, 7)):
        play, cldfr, alpha = _inputs(oracle, icld, wp)
        head, got = _drive(tmp, exe, icld, nsamp, step, irng, play, cldfr, alpha, device=False)
        _check(hip, head, got, icld, nsamp, step, irng, play, cldfr, alpha, wp)
        assert head[1] == head[0] and np.array_equal(got["tot2"], got["cldtot"])          # cldtot alone, by keyword


@needs_flang
@pytest.mark.gpu
@pytest.mark.parametrize("wp", [8, 4])
def test_device_entry_equals_the_python_entry(tmp_path, hip, oracle, wp):
    tmp = str(tmp_path)
    exe = _compile(tmp, wp, device=True)
    for icld, nsamp, step, irng in ((2, 1, 140, 0), (5, 3, 140, 0), (4, 1, 140, 1)):
        play, cldfr, alpha = _inputs(oracle, icld, wp)
        head, got = _drive(tmp, exe, icld, nsamp, step, irng, play, cldfr, alpha, device=True)
        assert head[1] == 0, "elements outside the call's columns were written"
        _check(hip, head, got, icld, nsamp, step, irng, play, cldfr, alpha, wp)
