"""The numpy restatement of the solver entry (tests/solve_ref.py) pinned to the reference's own Fortran through the column fixtures
tests/golden/ref_col_*.npz: taug and fracs are the fixture's (the reference's taumol), the Planck integrals a numpy setcoef, tauaer from
the input files, secdiff from the constants of tests/cloud_optics_ref.py and the column's precipitable water.  On the seven clear
fixtures every output is compared (-aer12 with its aerosol term, -idrv1 with dtotuflux_dt), on the two icld2 fixtures the clear-sky
stream.  Bound: solve_ref.FTOL = 1e-9 W m-2 for fluxes and heatfac * 2 * FTOL / |dp| for heating rates - fluxes below 700 W m-2 and a few
hundred rounded operations per g-point give a few 1e-11; if the restatement misses it, the restatement is wrong.  No GPU."""
import glob
import os
import sys

import numpy as np
import pytest

from rrtmg_lw_amd.io_rrtm import read_input_rrtm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_optics_ref as cor  # noqa: E402
import solve_ref as sr  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(glob.glob(os.path.join(G, "ref_col_*.npz")))


def column_inputs(f):
    """the solver entry's arrays (one column) of a fixture, and the prepared column"""
    j = lambda n: os.path.join(G, n) if n else None
    col = read_input_rrtm(j(str(f["inp"])), j(str(f["cld"])), j(str(f["aer"])))
    nl = int(col["nlayers"])
    s = cor.A0 + cor.A1 * np.exp(cor.A2 * float(col["pwvcm"]))
    sec = np.where(cor.FIXED, 1.66, np.minimum(np.maximum(s, 1.5), 1.8))
    band = sr.bands(140)
    tauaer = np.asarray(col["tauaer"], dtype=np.float64).reshape(nl, 16)
    tau = sec[band][None, :] * (np.asarray(f["taug"], dtype=np.float64) + tauaer[:, band])
    emis = np.asarray(col["semiss"], dtype=np.float64).reshape(1, 16)
    d = dict(ncol=1, nlay=nl, plev=np.asarray(col["pz"]).reshape(1, nl + 1), emis=emis, tau=tau[None], fracs=np.asarray(f["fracs"], dtype=np.float64)[None])
    d.update(sr.planck(np.asarray(col["tavel"]).reshape(1, nl), np.asarray(col["tz"]).reshape(1, nl + 1), np.array([float(col["tbound"])]), emis))
    return d, col


def test_there_are_nine_fixtures():
    names = [os.path.basename(p) for p in FIXTURES]
    assert len(names) == 9 and sum("icld2" in n for n in names) == 2, names


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_restatement_matches_the_reference_fortran(oracle, path):
    f = np.load(path)
    d, col = column_inputs(f)
    idrv = int(col["idrv"])
    got = sr.solve(oracle.luts(), d, cloud=0, idrv=idrv)
    clear = int(col["icld"]) == 0
    pairs = [("uflxc", "totuclfl"), ("dflxc", "totdclfl")] + ([("uflx", "totuflux"), ("dflx", "totdflux")] if clear else [])
    if idrv == 1:
        pairs += [("duflxc_dt", "dtotuclfl_dt")] + ([("duflx_dt", "dtotuflux_dt")] if clear else [])
    worst = 0.0
    for mine, theirs in pairs:
        e = float(np.abs(got[mine][0] - f[theirs]).max())
        worst = max(worst, e)
        print(f"{os.path.basename(path)}: max |{mine} - {theirs}| = {e:.3e} W m-2")
        assert e <= sr.FTOL, (mine, e)
    nl = int(col["nlayers"])
    bound = sr.hr_bound(d["plev"])[0]
    for mine, theirs in [("hrc", "htrc")] + ([("hr", "htr")] if clear else []):
        e = np.abs(got[mine][0] - f[theirs][:nl])
        print(f"{os.path.basename(path)}: max |{mine} - {theirs}| / bound = {float((e / bound).max()):.3e}")
        assert (e <= bound).all(), mine
    assert worst < 700.0
