"""rrtmg_lw_alpha_dev and rrtmg_lw_mcica_samples_dev of module rrtmg_lw_device from a flang-built, GPU-resident host model
(tests/fortran/drive_samples_dev.f90, built like tests/test_fortran_device.py builds its driver): fields (pcols = ncol + 5, nlay) in
device memory from hipMalloc, the call's columns from column 4 on, alpha made on the device and handed straight to the averaging
routine with the three variances.  Bit for bit api.get_alpha_device and api.rrtmg_lw_mcica_samples_device on contiguous tensors of the
host's real kind; the driver counts the elements outside the call's columns that no longer hold their NaN.
Also the optional variances of the host module rrtmg_lw_samples (tests/fortran/drive_samples_var.f90) against the Python host entry."""
import os
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import ArrayForm
from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")]

FLUX = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
VAR = ("uflx_var", "dflx_var", "hr_var")
GASES = ("h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr")
NCOL, NLAY, ICLD, SEED, NSAMP, STEP, IDCOR, JULDAT, DECORR = 70, 45, 5, 280, 3, 140, 1, 100, 2500.0


def _compile(tmp, wp):
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_device.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_samples_dev.o")
    subprocess.run([FLANG, "-cpp", f"-DWP={wp}", "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_samples_dev.f90"), "-o", drv], check=True, cwd=tmp)
    exe = os.path.join(tmp, "drive_samples_dev")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, cwd=tmp)
    return exe


def _drive(tmp, d, dz, lat, wp):
    """writes the inputs, runs the host model, returns (icld, dict of its outputs as float64 arrays)"""
    ncol, nlay = d["ncol"], d["nlay"]
    exe = _compile(tmp, wp)
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([ncol, nlay, ICLD, d["idrv"], d["inflglw"], d["iceflglw"], d["liqflglw"], SEED, NSAMP, STEP, IDCOR, JULDAT], dtype=np.int32).tofile(f)
        np.array([DECORR], dtype=np.float64).tofile(f)
        for k in ("play", "plev", "tlay", "tlev", "tsfc"):
            f.write(np.asfortranarray(d[k]).tobytes(order="F"))
        f.write(np.stack([d[k] for k in GASES], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(d["emis"]).tobytes(order="F"))
        f.write(np.stack([d[k] for k in ("cldfr", "cicewp", "cliqwp", "reice", "reliq")], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(d["taucld"]).tobytes(order="F"))
        f.write(np.asfortranarray(d["tauaer"]).tobytes(order="F"))
        f.write(np.asfortranarray(dz).tobytes(order="F"))
        f.write(np.asfortranarray(lat).tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    icld_out, nbad = (int(v) for v in np.frombuffer(raw, dtype=np.int32, count=2))
    assert nbad == 0, "elements outside the call's columns were written"
    a = np.frombuffer(raw, dtype=np.float64, offset=8)
    out, pos = {}, 0
    for k in FLUX + VAR + ("alpha",):
        shape = arrays.reference_shape(k, ncol, nlay)
        n = int(np.prod(shape))
        out[k] = a[pos:pos + n].reshape(shape, order="F")
        pos += n
    assert pos == a.size
    return icld_out, out


@pytest.mark.parametrize("wp", [8, 4])
def test_alpha_and_sample_statistics_from_a_device_resident_host(tmp_path, hip, wp):
    import torch
    d = make_gcm_inputs(NCOL, NLAY, "aer_idrv", col0=31)
    assert d["idrv"] == 1
    rng = np.random.default_rng(3)
    dz, lat = rng.uniform(100, 1500, (NCOL, NLAY)), rng.uniform(-90, 90, NCOL)
    ic, got = _drive(str(tmp_path), d, dz, lat, wp)
    form = ArrayForm(wp, 0, 0)
    x = arrays.from_reference(dict(d, dz=np.asfortranarray(dz), lat=lat), form)
    xd = {k: (torch.from_numpy(v).to("cuda:0") if isinstance(v, np.ndarray) else v) for k, v in x.items()}
    s = torch.cuda.current_stream().cuda_stream
    kw = {} if form.is_reference else {"form": form}
    alpha = arrays.empty_like_form(("alpha",), NCOL, NLAY, form, device="cuda:0", fill=float("nan"))["alpha"]
    hip.get_alpha_device(xd, alpha, ICLD, IDCOR, DECORR, JULDAT, stream=s, **kw)
    out = arrays.empty_like_form(FLUX + VAR, NCOL, NLAY, form, device="cuda:0", fill=float("nan"))
    ic2 = hip.rrtmg_lw_mcica_samples_device(xd, out, SEED, NSAMP, seedstep=STEP, alpha=alpha, icld=ICLD, stream=s, **kw)
    hip.check(s)
    assert ic == ic2
    want = {k: v.cpu().numpy().astype(np.float64) for k, v in dict(out, alpha=alpha).items()}
    for k in FLUX + VAR + ("alpha",):
        assert np.isfinite(want[k]).all() and np.array_equal(got[k], want[k]), k
    assert got["alpha"].max() > 0.1 and got["uflx_var"].max() > 1e-2


def test_host_module_returns_the_variances(tmp_path, hip):
    tmp = str(tmp_path)
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_samples.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_samples_var.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_samples_var.f90"), "-o", drv], check=True, cwd=tmp)
    exe = os.path.join(tmp, "drive_samples_var")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}"], check=True, cwd=tmp)
    ncol, nlay, icld = 70, 40, 2
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=31)
    alpha = np.zeros((ncol, nlay))
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([ncol, nlay, icld, d["idrv"], d["inflglw"], d["iceflglw"], d["liqflglw"], SEED, NSAMP, STEP, 0], dtype=np.int32).tofile(f)
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
    want = hip.rrtmg_lw_mcica_subcol_from_dict(d, SEED, 0, alpha=alpha, icld=icld, nsamp=NSAMP, seedstep=STEP, var=True)
    assert icld_out == want["icld"]
    pos = 0
    for k in FLUX + VAR + ("hr_var",):
        n = ncol * (nlay if k.startswith("hr") else nlay + 1)
        got = a[pos:pos + n].reshape((ncol, n // ncol), order="F")
        pos += n
        if not k.startswith("du"):               # (idrv = 0: the derivatives are not written)
            assert np.array_equal(got, want[k]), k
    assert pos == a.size and want["hr_var"].max() > 1e-2
