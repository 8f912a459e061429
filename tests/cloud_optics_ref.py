"""What rrtmg_lw_hip_cloud_optics* must return, from the definitions in include/rrtmg_lw_hip.h: a numpy restatement of cldprop's
(imca = 0, src/rrtmg_lw_cldprop.f90:173-293 with rtrn's band -> cloud-band map, src/rrtmg_lw_rtrn.f90:343-349) and cldprmc's (imca = 1,
src/rrtmg_lw_cldprmc.f90:173-273 on a cloudy sub-column) optical depth per spectral band, of cldprop's band count and of the diffusivity
secants (rtrn :280-288 from inatm's pwvcm), built on cloud_states.decisions / ice_position / liq_position.  Every operation is a
float64 numpy operation that rounds on its own, in the order the header states.  A helper module (not a conftest) for
tests/test_cloud_optics_ref.py, which pins it to the oracle, and tests/test_hip_cloud_optics.py.  No GPU, no library."""
import numpy as np

import cloud_states as cs

NBND = 16
# secdiff = A0 + A1 * exp(A2 * pwvcm) in the bands where A1 != 0 (rtrn :265-288)
A0 = np.array([1.66, 1.55, 1.58, 1.66, 1.54, 1.454, 1.89, 1.33, 1.668, 1.66, 1.66, 1.66, 1.66, 1.66, 1.66, 1.66])
A1 = np.array([0.00, 0.25, 0.22, 0.00, 0.13, 0.446, -0.10, 0.40, -0.006, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00])
A2 = np.array([0.00, -12.0, -11.7, 0.00, -0.72, -0.243, 0.19, -0.062, 0.414, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00])
FIXED = np.array([b in (1, 4) or b >= 10 for b in range(1, NBND + 1)])         # bands whose secant is 1.66 whatever the water


def icb(ncbands):
    """the cloud band ib = ipat(B, .) of every spectral band B for a column's band count (cldprop :167-169, rtrn :343-349), 1-based"""
    return cs.ICB[{1: 0, 5: 1, 16: 2}[int(ncbands)]]


def ncbands(d, imca=0):
    """(ncol,) int32: cldprop's band count at the end of the column; 16 for cldprmc, which carries none"""
    if imca:
        return np.full(int(d["ncol"]), NBND, dtype=np.int32)
    return cs.decisions(d)["nb_final"][:, 0].astype(np.int32)


def _arrays(d):
    return [np.asarray(d[k], dtype=np.float64) for k in ("cldfr", "cicewp", "cliqwp", "reice", "reliq", "taucld")]


def _interp(tb, position):
    i, f = position
    return tb[i - 1] + f * (tb[i] - tb[i - 1])


def taucloud(d, imca=0):
    """(ncol, nlay, 16) float64, Fortran-ordered; zeros in the cells of a stop (the library's outputs are not valid there)"""
    return _taucloud_mc(d) if imca else _taucloud_prop(d)


def _taucloud_prop(d):
    inflag, iceflag, liqflag = int(d["inflglw"]), int(d["iceflglw"]), int(d["liqflglw"])
    cf, ciwp, clwp, rei, rel, taucld = _arrays(d)
    dec = cs.decisions(d)
    out = np.zeros(cf.shape + (NBND,), order="F")
    for i, l in zip(*np.nonzero(dec["enters"] & (dec["stop"] == 0))):
        nb_at, bands = int(dec["nb_at"][i, l]), icb(dec["nb_final"][i, l])
        wi, wl = ciwp[i, l], clwp[i, l]
        if inflag == 2:
            iceind, liqind = int(dec["iceind"][i, l]), int(dec["liqind"][i, l])
            if wi == 0.0:
                ai = np.zeros(NBND)                                                 # abscoice(1) = 0, iceind 0
            elif iceflag == 0:
                ai = np.full(NBND, cs.ABSICE0[0] + cs.ABSICE0[1] / rei[i, l])
            elif iceflag == 1:
                ai = cs.ABSICE1[0] + cs.ABSICE1[1] / rei[i, l]                      # five Ebert-Curry bands
            else:
                ai = _interp(cs.ABSICE2 if iceflag == 2 else cs.ABSICE3, cs.ice_position(iceflag, rei[i, l]))
            if wl == 0.0:
                al = np.zeros(NBND)
            elif liqflag == 0:
                al = np.full(NBND, cs.ABSLIQ0)
            else:
                al = _interp(cs.ABSLIQ1, cs.liq_position(rel[i, l]))
        for B in range(1, NBND + 1):
            ib = int(bands[B - 1])
            if ib > nb_at:              # not assigned while cldprop carried fewer bands
                continue
            if inflag == 0:
                out[i, l, B - 1] = taucld[ib - 1, i, l]
            elif inflag == 1:
                out[i, l, B - 1] = cs.ABSCLD1 * (wi + wl)
            elif inflag == 2:
                ki, kl = int(cs.ICB[iceind][ib - 1]), int(cs.ICB[liqind][ib - 1])
                if iceflag == 1 and wi != 0.0:
                    ki = min(ki, 5)     # the library's stated deviation: an ice-only Ebert-Curry layer of a 16-band column (k_cloudlay)
                out[i, l, B - 1] = wi * ai[ki - 1] + wl * al[kl - 1]
    return out


def _taucloud_mc(d):
    inflag, iceflag, liqflag = int(d["inflglw"]), int(d["iceflglw"]), int(d["liqflglw"])
    cf, ciwp, clwp, rei, rel, taucld = _arrays(d)
    out = np.zeros(cf.shape + (NBND,), order="F")
    for i, l in zip(*np.nonzero(cf >= cs.CLDMIN)):
        wi, wl = ciwp[i, l], clwp[i, l]
        tb = taucld[:, i, l]
        enters = ((wi + wl) >= cs.CLDMIN) | (tb >= cs.CLDMIN)                      # cldprmc :181-183, per cell
        out[i, l] = tb                                                              # a cell that does not enter keeps its taucld
        if not enters.any() or inflag == 0:
            continue
        if inflag == 1:
            raise ValueError("INFLAG = 1 OPTION NOT AVAILABLE WITH MCICA")
        ai = np.zeros(NBND) if wi == 0.0 else cs.ice_coef(iceflag, rei[i, l])      # (iceflag 1: the five-band map per band)
        al = np.zeros(NBND) if wl == 0.0 else cs.liq_coef(liqflag, rel[i, l])
        out[i, l] = np.where(enters, wi * ai + wl * al, tb)
    return out


def pwvcm(d):
    """(ncol,) precipitable water in cm, inatm (src/rrtmg_lw_rad.nomcica.f90:795-863): needs plev and h2ovmr only"""
    amd, amw, avogad, grav = 28.9660, 18.0160, 6.02214199e+23, 9.8066
    plev, h2o = np.asarray(d["plev"], dtype=np.float64), np.asarray(d["h2ovmr"], dtype=np.float64)
    amttl, wvttl = np.zeros(plev.shape[0]), np.zeros(plev.shape[0])
    for l in range(h2o.shape[1]):
        w = h2o[:, l]
        amm = (1. - w) * amd + w * amw
        coldry = (plev[:, l] - plev[:, l + 1]) * 1.e3 * avogad / (1.e2 * grav * amm * (1. + w))
        amttl = amttl + coldry + coldry * w
        wvttl = wvttl + coldry * w
    wvsh = (amw * wvttl) / (amd * amttl)
    return wvsh * (1.e3 * plev[:, 0]) / (1.e2 * grav)


def secdiff(d):
    """(ncol, 16) float64, Fortran-ordered: exactly 1.66 in bands 1, 4 and 10-16, clamped to [1.5, 1.8] elsewhere"""
    s = A0 + A1 * np.exp(A2 * pwvcm(d)[:, None])
    s = np.minimum(np.maximum(s, 1.5), 1.8)
    return np.asfortranarray(np.where(FIXED, 1.66, s))


def cloud_band_secdiff(sec, nb):
    """(ncol, 16): secdiff(icb(B, ncbands)) - the secant the DETERMINISTIC solver applies to taucloud(B): the reference indexes secdiff
    by the cloud band (rtrn :323)"""
    return np.stack([sec[i, icb(nb[i]) - 1] for i in range(sec.shape[0])])
