"""The numpy restatement of the cloud-optics outputs (tests/cloud_optics_ref.py) pinned to the oracle, and through it to the reference's
Fortran: with taucld replaced by the restated taucloud and inflglw = 0 - cldprop / cldprmc then pass the optical depths through - the
oracle must return the fluxes and heating rates of the original call BIT FOR BIT, on the designed cloud states (tests/cloud_states.py).

imca = 0, columns whose ncbands is 16: the broadband results of every call of families A and B, icld 1 and 2.
imca = 0, columns whose ncbands is 1 or 5: the broadband closure cannot hold - rtrn scales taucloud with secdiff of the CLOUD band
  (src/rrtmg_lw_rtrn.f90:323), and the replaced call has 16 cloud bands - so these close per band, in the bands whose cloud band has the
  band's own secant: 1, 4 and 10-15 for ncbands = 1 (cloud band 1, 1.66 like theirs), 1-3 for ncbands = 5 (cloud bands 1, 2, 3).  Cloud
  bands 4 and 5 of the five-band map cannot be closed this way (their spectral bands 6-8 and 9-16 carry other secants than bands 4 and
  5); they share the code of bands 1-3 (one expression indexed by the band).  At most PER_CALL columns per call: one oracle run per band.
imca = 1: the sub-columns of the oracle's generator with taucmcl = cldfmcl * taucloud[band of g]: every column of every call of family
  A and of the inflglw = 2 calls of family B, icld 1-3.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_optics_ref as cor  # noqa: E402
import cloud_states as cs  # noqa: E402
from test_cloud_state_coverage import FLUX_KEYS, subcolumns  # noqa: E402
from test_hip_spectral import inatm  # noqa: E402
from rrtmg_lw_amd.kspec import NGC  # noqa: E402

OUT = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
PER_CALL = 40
BAND_OF_G = np.repeat(np.arange(16), NGC)            # spectral band (0-based) of each of the 140 g-points
OWN_SECANT = {1: (1, 4, 10, 11, 12, 13, 14, 15), 5: (1, 2, 3)}


@pytest.fixture(scope="module")
def calls():
    c = {("A",) + k: v for k, v in cs.family_a().items()}
    c.update({("B",) + k: v for k, v in cs.family_b().items()})
    return c


def as_taucld(tau):
    """(ncol, nlay, 16) -> taucld's (16, ncol, nlay)"""
    return np.asfortranarray(np.moveaxis(tau, 2, 0))


def test_restatement_shapes_and_zeros(calls):
    """zero outside the layers that enter; cloud bands above the count in effect at the layer stay zero; ncbands is 1, 5 or 16"""
    seen = set()
    for key, d in calls.items():
        dec, tau, nb = cs.decisions(d), cor.taucloud(d), cor.ncbands(d)
        assert tau.shape == (d["ncol"], d["nlay"], 16) and nb.dtype == np.int32 and set(np.unique(nb)) <= {1, 5, 16}
        assert not tau[~dec["enters"]].any()
        late = dec["enters"] & (dec["nb_at"] < dec["nb_final"])
        for i, l in zip(*np.nonzero(late)):
            ib = cor.icb(nb[i])
            assert not tau[i, l][ib > dec["nb_at"][i, l]].any() and tau[i, l][ib <= dec["nb_at"][i, l]].all(), d["labels"][i]
            seen.add((int(dec["nb_at"][i, l]), int(nb[i])))
    assert seen == {(1, 5), (1, 16), (5, 16)}


@pytest.mark.parametrize("icld", (1, 2))
def test_sixteen_band_columns_close_broadband(oracle, calls, icld):
    n = 0
    for key, d in calls.items():
        idx = np.nonzero(cor.ncbands(d) == 16)[0]
        if not idx.size:
            continue
        sub = cs.take(d, idx)
        rep = cs.with_arrays(sub, taucld=as_taucld(cor.taucloud(sub)))
        rep["inflglw"] = 0
        a, b = oracle.rrtmg_lw(sub["ncol"], sub["nlay"], icld, 0, sub), oracle.rrtmg_lw(sub["ncol"], sub["nlay"], icld, 0, rep)
        for k in OUT:
            bad = np.nonzero((a[k] != b[k]).any(axis=1))[0]
            assert not bad.size, (key, icld, k, len(bad), sub["labels"][int(bad[0])], float(np.abs(a[k] - b[k]).max()))
        n += idx.size
    assert n > 1500


@pytest.mark.parametrize("key", ((2, 0, 0), (2, 1, 0), (2, 1, 1)))
def test_one_and_five_band_columns_close_per_band(oracle, key):
    d = cs.family_b()[key]
    nb = cor.ncbands(d)
    idx = np.nonzero(nb != 16)[0][:PER_CALL]
    assert idx.size >= 10
    rep = cs.with_arrays(d, taucld=as_taucld(cor.taucloud(d)))
    rep["inflglw"] = 0
    runs = 0
    for i in idx:
        ca, cb = inatm(d, int(i), 2), inatm(rep, int(i), 2)
        for band in OWN_SECANT[int(nb[i])]:
            a, b = oracle.column(ca, band, band, iout=99), oracle.column(cb, band, band, iout=99)
            for k in FLUX_KEYS:
                assert np.array_equal(a[k], b[k]), (key, d["labels"][int(i)], band, k, float(np.abs(a[k] - b[k]).max()))
            runs += 1
    assert runs >= 3 * idx.size


@pytest.mark.parametrize("icld", (1, 2, 3))
def test_mcica_columns_close(oracle, calls, icld):
    for key, d in calls.items():
        if int(d["inflglw"]) != 2:
            continue
        sc = subcolumns(oracle, d, icld)
        tau = cor.taucloud(d, imca=1)                                               # (ncol, nlay, 16)
        rep = dict(sc, inflglw=0, taucmcl=np.asfortranarray(sc["cldfmcl"] * np.moveaxis(tau, 2, 0)[BAND_OF_G]))
        a, b = oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, 0, sc, mcica=True), oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, 0, rep, mcica=True)
        for k in OUT:
            bad = np.nonzero((a[k] != b[k]).any(axis=1))[0]
            assert not bad.size, (key, icld, k, len(bad), d["labels"][int(bad[0])], float(np.abs(a[k] - b[k]).max()))


def test_mcica_cells_that_do_not_enter_keep_their_taucld(calls):
    """family B's 1e-25 water paths: a band whose taucld is below 1e-20 keeps it, whatever the flags; and inflglw = 1 is the stop"""
    hit = 0
    for key, d in calls.items():
        if key[0] != "B" or int(d["inflglw"]) != 2:
            continue
        tau = cor.taucloud(d, imca=1)
        cwp = np.asarray(d["cicewp"]) + np.asarray(d["cliqwp"])
        keep = (np.asarray(d["cldfr"]) >= cs.CLDMIN) & (cwp < cs.CLDMIN) & (np.asarray(d["taucld"]) < cs.CLDMIN).all(axis=0)
        assert np.array_equal(tau[keep], np.moveaxis(np.asarray(d["taucld"]), 0, 2)[keep])
        hit += int(keep.sum())
    assert hit > 0
    with pytest.raises(ValueError, match="INFLAG = 1"):
        cor.taucloud(cs.family_b()[(1, 0, 0)], imca=1)


def test_secdiff_restatement():
    from rrtmg_lw_amd.synth import make_gcm_inputs
    d = make_gcm_inputs(40, 30, "clear")
    s = cor.secdiff(d)
    assert s.shape == (40, 16) and (s[:, cor.FIXED] == 1.66).all() and (s >= 1.5).all() and (s <= 1.8).all()
    assert np.ptp(s[:, ~cor.FIXED], axis=0).max() > 0 or (cor.pwvcm(d) > 0).all()
