"""The Fortran shims' optional spectral dummies (uflxs, dflxs, uflxcs, dflxcs): both shim flavours compile with them (no GPU), and a
flang host model that passes them gets what api.rrtmg_lw(..., spectral=True) returns, bit for bit (tests/fortran/drive_spectral.f90)."""
import os
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")

# a host that passes the optionals by keyword, with the McICA shim: compiles against the module's interface
MCICA_CALLER = """
subroutine host_step(ncol, nlay, play, plev, tlay, tlev, tsfc, gas, emis, cfm, tcm, cim, clm, rim, rlm, tauaer, &
                     uflx, dflx, hr, uflxc, dflxc, hrc, us, ds, ucs, dcs)
  use parkind, only: im => kind_im, rb => kind_rb
  use rrtmg_lw_rad, only: rrtmg_lw
  implicit none
  integer(im), intent(in) :: ncol, nlay
  real(rb), intent(in) :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), gas(:,:,:), emis(:,:)
  real(rb), intent(in) :: cfm(:,:,:), tcm(:,:,:), cim(:,:,:), clm(:,:,:), rim(:,:), rlm(:,:), tauaer(:,:,:)
  real(rb), intent(out) :: uflx(:,:), dflx(:,:), hr(:,:), uflxc(:,:), dflxc(:,:), hrc(:,:)
  real(rb), intent(out) :: us(:,:,:), ds(:,:,:), ucs(:,:,:), dcs(:,:,:)
  integer(im) :: icld
  icld = 2
  call rrtmg_lw(ncol, nlay, icld, 0, play, plev, tlay, tlev, tsfc, gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), &
                gas(:,:,5), gas(:,:,6), gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), emis, 2, 3, 1, &
                cfm, tcm, cim, clm, rim, rlm, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
                uflxs=us, dflxs=ds, uflxcs=ucs, dflxcs=dcs)
  call rrtmg_lw(ncol, nlay, icld, 0, play, plev, tlay, tlev, tsfc, gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), &
                gas(:,:,5), gas(:,:,6), gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), emis, 2, 3, 1, &
                cfm, tcm, cim, clm, rim, rlm, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, uflxs=us, dflxs=ds)
end subroutine host_step
"""


def _compile_shim(tmp, mcica):
    shim = ("parkind.f90", "rrtmg_lw_init.f90", "mcica_subcol_gen_lw.f90", "rrtmg_lw_rad.f90") if mcica else \
           ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_rad.nomcica.f90")
    objs = []
    for f in shim:
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    return objs


@needs_flang
def test_both_shims_compile_with_the_spectral_optionals(tmp_path):
    nomc, mc = tmp_path / "nomcica", tmp_path / "mcica"
    nomc.mkdir()
    mc.mkdir()
    _compile_shim(str(nomc), False)
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_spectral.f90"), "-o", str(nomc / "d.o")],
                   check=True, cwd=str(nomc))
    _compile_shim(str(mc), True)
    (mc / "host.f90").write_text(MCICA_CALLER)
    subprocess.run([FLANG, "-c", "-O2", "host.f90", "-o", "host.o"], check=True, cwd=str(mc))
    for d in (nomc, mc):
        assert b"rrtmg_lw_hip_run_" in open(d / "rrtmg_lw_rad.f90.o" if (d / "rrtmg_lw_rad.f90.o").exists()
                                             else d / "rrtmg_lw_rad.nomcica.f90.o", "rb").read()
    syms = subprocess.run(["nm", str(nomc / "rrtmg_lw_rad.nomcica.f90.o")], capture_output=True, text=True).stdout
    assert "rrtmg_lw_hip_run_nomcica_spectral" in syms
    syms = subprocess.run(["nm", str(mc / "rrtmg_lw_rad.f90.o")], capture_output=True, text=True).stdout
    assert "rrtmg_lw_hip_run_mcica_spectral" in syms


@needs_flang
@pytest.mark.gpu
@pytest.mark.parametrize("config,icld", [("cloudy", 2), ("aer_idrv", 1)])
def test_fortran_host_model_spectral_matches_python(tmp_path, hip, config, icld):
    tmp = str(tmp_path)
    objs = _compile_shim(tmp, False)
    drv = os.path.join(tmp, "drive_spectral.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_spectral.f90"), "-o", drv], check=True, cwd=tmp)
    exe = os.path.join(tmp, "drive_spectral")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}"], check=True, cwd=tmp)
    ncol, nlay = 96, 60
    d = make_gcm_inputs(ncol, nlay, config, col0=31)
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([ncol, nlay, icld, d["idrv"], d["inflglw"], d["iceflglw"], d["liqflglw"]], dtype=np.int32).tofile(f)
        for k in ("play", "plev", "tlay", "tlev", "tsfc"):
            f.write(np.asfortranarray(d[k]).tobytes(order="F"))
        gases = ["h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr"]
        f.write(np.stack([d[k] for k in gases], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(d["emis"]).tobytes(order="F"))
        f.write(np.stack([d[k] for k in ("cldfr", "cicewp", "cliqwp", "reice", "reliq")], axis=2).tobytes(order="F"))
        f.write(np.asfortranarray(d["taucld"]).tobytes(order="F"))
        f.write(np.asfortranarray(d["tauaer"]).tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    a = np.frombuffer(raw, dtype=np.float64, offset=4)
    want = hip.rrtmg_lw_from_dict(d, icld=icld, spectral=True)
    pos = 0
    for k, shape in (("uflx", (ncol, nlay + 1)), ("dflx", (ncol, nlay + 1)), ("hr", (ncol, nlay)), ("uflxc", (ncol, nlay + 1)),
                     ("dflxc", (ncol, nlay + 1)), ("hrc", (ncol, nlay)), ("uflxs", (ncol, nlay + 1, 16)), ("dflxs", (ncol, nlay + 1, 16)),
                     ("uflxcs", (ncol, nlay + 1, 16)), ("dflxcs", (ncol, nlay + 1, 16))):
        n = int(np.prod(shape))
        got = a[pos:pos + n].reshape(shape, order="F")
        pos += n
        assert np.array_equal(got, want[k]), k
