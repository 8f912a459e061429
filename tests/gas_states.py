"""A designed set of gas states for the gas-optics tests (a helper module, not a conftest).

Every other input of the suite descends from the mid-latitude-summer profile with MLS gas ratios, which keeps taumol's binary-species
parameter near 0.5 in every band.  This module builds columns BY CONSTRUCTION from target values of what setcoef and taumol decide:

  decisions(d)            numpy / float64 restatement of those decisions per (column, layer) - no optical depths
  make_gas_states(...)    GCM-interface inputs (the dict of rrtmg_lw_amd.synth.make_gcm_inputs) that reach every branch: a grid of
                          specparm values for every ratio of every binary band, both sides of the minor-gas adjustment thresholds,
                          layer pressures above the first reference pressure and below the last, temperatures beyond both table ends,
                          zero gas amounts
  prepared_companion(...) prepared columns (the column entries) with CO and the halocarbon amounts varied, which the GCM interface cannot

Written from SURVEY.md appendix B and src/rrtmg_lw_setcoef.f90:276-412 / src/rrtmg_lw_taumol.f90 of the reference.
"""
import os

import numpy as np

from rrtmg_lw_amd.blob import read_blob
from rrtmg_lw_amd.synth import NBND, base_profile, make_gcm_inputs

_STATIC = read_blob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rrtmg_lw_amd", "data", "lw_static.bin"))
CHI = np.asarray(_STATIC["chi_mls"], dtype=np.float64).reshape(7, 59)        # CHI[species - 1, reference level - 1]
PREFLOG = np.asarray(_STATIC["preflog"], dtype=np.float64)
TREF = np.asarray(_STATIC["tref"], dtype=np.float64)
ONEMINUS = 1.0 - 1.0e-6
AMD, AMW, AVOGAD, GRAV = 28.9660, 18.0160, 6.02214199e23, 9.8066
H2O, CO2, O3, N2O, CO, CH4, O2 = range(7)
VMR_KEY = {H2O: "h2ovmr", CO2: "co2vmr", O3: "o3vmr", N2O: "n2ovmr", CH4: "ch4vmr", O2: "o2vmr"}
NAME = {H2O: "h2o", CO2: "co2", O3: "o3", N2O: "n2o", CO: "co", CH4: "ch4", O2: "o2"}

# band, region, first and second species of the key, reference level of the Planck ratio, {minor-gas ratio: reference level}
BINARY = (
    (3, "lower", H2O, CO2, 9, {"jmn2o": 3}), (3, "upper", H2O, CO2, 13, {"jmn2o": 13}),
    (4, "lower", H2O, CO2, 11, {}), (4, "upper", O3, CO2, 13, {}),
    (5, "lower", H2O, CO2, 5, {"jmo3": 7}), (5, "upper", O3, CO2, 43, {}),
    (7, "lower", H2O, O3, 3, {"jmco2": 3}),
    (9, "lower", H2O, CH4, 9, {"jmn2o": 3}),
    (12, "lower", H2O, CO2, 10, {}),
    (13, "lower", H2O, N2O, 5, {"jmco2": 1, "jmco": 3}),
    (15, "lower", N2O, CO2, 1, {"jmn2": 1}),
    (16, "lower", H2O, CH4, 6, {}),
)
# band, region, gas, threshold of 1e20 (col / coldry) / chi_ref, chi_ref (None: chi_mls(gas, jp + 1))
THRESHOLDS = (
    (3, "lower", N2O, 1.5, None), (3, "upper", N2O, 1.5, None), (6, "lower", CO2, 3.0, None), (7, "lower", CO2, 3.0, None),
    (7, "upper", CO2, 3.0, None), (8, "lower", CO2, 3.0, None), (8, "upper", CO2, 3.0, None), (9, "lower", N2O, 1.5, None),
    (9, "upper", N2O, 1.5, None), (13, "lower", CO2, 3.0, 3.55e-4),
)


def _coldry(d):
    """inatm's dry-air column per layer (src/rrtmg_lw_rad.nomcica.f90:760-764)"""
    plev, h2o = np.asarray(d["plev"], dtype=np.float64), np.asarray(d["h2ovmr"], dtype=np.float64)
    amm = (1.0 - h2o) * AMD + h2o * AMW
    return (plev[:, :-1] - plev[:, 1:]) * 1.e3 * AVOGAD / (1.e2 * GRAV * amm * (1.0 + h2o))


def _spec(cola, rat, colb, mult):
    with np.errstate(invalid="ignore", divide="ignore"):
        specparm = np.minimum(cola / (cola + rat * colb), ONEMINUS)
    return specparm, 1 + np.trunc(mult * specparm).astype(np.int64)


def decisions(d):
    """What setcoef and taumol decide for every (column, layer) of the GCM inputs d.  Returns a dict of (ncol, nlay) arrays:
    lower (bool: below laytrop), jp, jt, jt1, indself (0 above laytrop), indfor, indminor, fp, regime (2: plog > 5.76, 1: > 4.56, 0:
    neither), and two dicts:
      spec[(band, region, kind)] = (specparm, js)   kind: "main", "jp1", "planck" or a minor-gas ratio ("jmn2o", "jmco2", "jmo3", "jmco",
                                                    "jmn2"); NaN / 0 outside the region
      adj[(band, region)] = (ratio, above)          ratio: 1e20 (col / coldry) / chi_ref, above: ratio > threshold; NaN / False outside"""
    play, tlay = np.asarray(d["play"], dtype=np.float64), np.asarray(d["tlay"], dtype=np.float64)
    coldry = _coldry(d)
    col = {}
    for m, k in VMR_KEY.items():
        col[m] = 1.e-20 * (coldry * np.asarray(d[k], dtype=np.float64))
    col[CO] = np.zeros_like(coldry)                                        # the GCM interface has no CO
    for m in (CO2, O3, N2O, CO, CH4):
        col[m] = np.where(col[m] == 0.0, 1.e-32 * coldry, col[m])          # setcoef :354-366
    plog = np.log(play)
    jp = np.clip(np.trunc(36.0 - 5 * (plog + 0.04)).astype(np.int64), 1, 58)
    fp = 5.0 * (PREFLOG[jp - 1] - plog)
    lower = ~(plog <= 4.56)
    jt = np.clip(np.trunc(3.0 + (tlay - TREF[jp - 1]) / 15.0).astype(np.int64), 1, 4)
    jt1 = np.clip(np.trunc(3.0 + (tlay - TREF[jp]) / 15.0).astype(np.int64), 1, 4)
    indfor = np.where(lower, np.minimum(2, np.maximum(1, np.trunc((332.0 - tlay) / 36.0).astype(np.int64))), 3)
    indself = np.where(lower, np.minimum(9, np.maximum(1, np.trunc((tlay - 188.0) / 7.2).astype(np.int64) - 7)), 0)
    indminor = np.minimum(18, np.maximum(1, np.trunc((tlay - 180.8) / 7.2).astype(np.int64)))
    regime = np.where(plog > 5.76, 2, np.where(plog > 4.56, 1, 0))
    out = dict(lower=lower, jp=jp, jt=jt, jt1=jt1, indself=indself, indfor=indfor, indminor=indminor, fp=fp, regime=regime, plog=plog)
    spec = {}
    for band, region, a, b, planck, minors in BINARY:
        inreg = lower if region == "lower" else ~lower
        mult = 8.0 if region == "lower" else 4.0
        rats = dict(main=CHI[a][jp - 1] / CHI[b][jp - 1], jp1=CHI[a][jp] / CHI[b][jp], planck=CHI[a][planck - 1] / CHI[b][planck - 1])
        rats.update({k: CHI[a][lev - 1] / CHI[b][lev - 1] for k, lev in minors.items()})
        for kind, rat in rats.items():
            sp, js = _spec(col[a], rat, col[b], mult)
            spec[(band, region, kind)] = (np.where(inreg, sp, np.nan), np.where(inreg, js, 0))
    adj = {}
    for band, region, gas, thr, chiref in THRESHOLDS:
        inreg = lower if region == "lower" else ~lower
        ref = CHI[gas][jp] if chiref is None else chiref
        ratio = 1.e20 * (col[gas] / coldry) / ref
        adj[(band, region)] = (np.where(inreg, ratio, np.nan), inreg & (ratio > thr))
    out.update(spec=spec, adj=adj)
    return out


def decision_row(dec, i, lay):
    """the decisions of cell (column i, layer index lay) as a short dict, for failure messages"""
    row = {k: (bool(dec[k][i, lay]) if k == "lower" else float(dec[k][i, lay]) if k in ("fp", "plog") else int(dec[k][i, lay]))
           for k in ("lower", "jp", "jt", "jt1", "indself", "indfor", "indminor", "fp", "regime")}
    for key, (sp, js) in dec["spec"].items():
        if js[i, lay]:
            row["b%d %s" % (key[0], key[2])] = (float(sp[i, lay]), int(js[i, lay]))
    for key, (ratio, above) in dec["adj"].items():
        if np.isfinite(ratio[i, lay]):
            row["b%d adj" % key[0]] = (float(ratio[i, lay]), bool(above[i, lay]))
    return row


# ------------------------------------------------------------------------------------------------------------------ the design
# Exact branch thresholds (0.125, 0.875) are left out: the stencils are continuous there and a last-bit difference in the quotient may
# legitimately pick the other branch.  The near-threshold values lie within 1e-3 of the threshold and no closer than 1e-6.
NEAR = (0.1242, 0.12493, 0.12507, 0.1258, 0.8742, 0.87493, 0.87507, 0.8758)
MIDS = {"lower": tuple((k + 0.5) / 8 for k in range(8)), "upper": (0.11, 0.375, 0.625, 0.89)}      # every js interval, low and high ends
CLAMP = "clamp"                                            # second species zero (setcoef's 1e-32 floor): specparm capped at oneminus
REPLICAS = ((1.0, 0.0), (0.8, 8.0))                        # surface-pressure factor, temperature offset: every design point twice
ADJ_FACTORS = (0.95, 1.05, 2.5)                            # of the threshold
HIGH_PS = (1060.0, 1065.0, 1070.0, 1075.0, 1080.0, 1085.0)
RAGGED_END = 300                                           # see make_gas_states
P_FIRST_REF = 1054.5                                      # just above exp(preflog(1)) = 1053.6 hPa: the layers below it have fp < 0


def _keys():
    """(first species, second species, region) -> sorted reference levels of its Planck and minor-gas ratios"""
    keys = {}
    for band, region, a, b, planck, minors in BINARY:
        keys.setdefault((a, b, region), set()).update([planck, *minors.values()])
    return {k: sorted(v) for k, v in keys.items()}


def _recipes():
    """the design points, each a dict; every one is built once per replica"""
    rs = []
    for (a, b, region), refs in _keys().items():
        for kind in ("main", "jp1"):
            for s in (0.0,) + NEAR + MIDS[region] + (CLAMP,):
                rs.append(dict(type="spec", a=a, b=b, region=region, kind=kind, s=s))
        for ref in refs:
            for s in (0.0,) + MIDS[region] + (CLAMP,):
                rs.append(dict(type="spec", a=a, b=b, region=region, kind=ref, s=s))
    for gas, thr, ref in ((CO2, 3.0, None), (CO2, 3.0, 3.55e-4), (N2O, 1.5, None)):
        for f in ADJ_FACTORS:
            rs.append(dict(type="adj", gas=gas, thr=thr, ref=ref, f=f))
    for gas in (O3, CH4, N2O, O2, H2O):
        rs.append(dict(type="zero", gas=gas))
    for dt in (-70.0, 70.0):
        rs.append(dict(type="plain", grid="std", dt=dt))
    rs.append(dict(type="plain", grid="allupper", dt=0.0))
    rs.append(dict(type="plain", grid="alllower", dt=0.0))
    return rs


def _class(r):
    """grouped order: the columns of one stencil branch side by side"""
    if r["type"] != "spec":
        return 3
    s = r["s"]
    return 2 if s == CLAMP or s > 0.875 else (0 if s < 0.125 else 1)


def _label(r):
    if r["type"] == "spec":
        kind = r["kind"] if isinstance(r["kind"], str) else "ref%d" % r["kind"]
        return "%s/%s %s %s s=%s" % (NAME[r["a"]], NAME[r["b"]], r["region"], kind, r["s"])
    if r["type"] == "adj":
        return "%s at %.2f x threshold%s" % (NAME[r["gas"]], r["f"], "" if r["ref"] is None else " (band 13)")
    if r["type"] == "zero":
        return "%s = 0" % NAME[r["gas"]]
    if r["type"] == "high":
        return "surface at %.0f hPa" % r["ps"]
    if r["type"] == "fill":
        return "MLS gases, surface-pressure factor %.3f" % r["psf"]
    return "MLS gases, %s grid, dT = %+.0f K" % (r["grid"], r["dt"])


def _levels(nlay, r, psf):
    """interface pressures of one column, surface first"""
    bp = base_profile(nlay)
    if r["type"] == "high":
        # two thin layers wholly above the first reference pressure, the rest log-spaced to the usual top
        return np.concatenate([np.linspace(r["ps"], P_FIRST_REF, 3), np.exp(np.linspace(np.log(P_FIRST_REF), np.log(0.067), nlay - 1))[1:]])
    grid = r.get("grid", "std")
    if grid == "std":
        return bp["plev"] * (r["psf"] if r["type"] == "fill" else psf)
    lo, hi = (np.log(1013.0), np.log(110.0)) if grid == "alllower" else (np.log(90.0), np.log(0.006))
    x = (np.log(bp["plev"]) - np.log(1013.0)) / (np.log(0.067) - np.log(1013.0))
    return np.exp(lo + x * (hi - lo)) * psf


def _column(nlay, r, psf, dt):
    """one column: pressures, temperatures and the MLS gases read at the column's own pressures, then the recipe's gases"""
    bp = base_profile(nlay)
    plev = _levels(nlay, r, psf)
    play = 0.5 * (plev[:-1] + plev[1:])
    at = lambda x, xp, f: np.interp(-np.log(x), -np.log(xp), f)
    dt = dt + r.get("dt", 0.0)
    tlay, tlev = at(play, bp["play"], bp["tlay"]) + dt, at(plev, bp["plev"], bp["tlev"]) + dt
    vmr = {m: at(play, bp["play"], bp["vmr"][m]) for m in (H2O, CO2, O3, N2O, CH4, O2)}
    plog = np.log(play)
    jp = np.clip(np.trunc(36.0 - 5 * (plog + 0.04)).astype(np.int64), 1, 58)
    lower = ~(plog <= 4.56)
    if r["type"] == "spec":
        a, b = r["a"], r["b"]
        inreg = lower if r["region"] == "lower" else ~lower
        if r["s"] == CLAMP:
            # second species zero -> setcoef's floor 1e-32 coldry, and specparm = 1 / (1 + 1e-12 rat / vmr_a): at or above oneminus only
            # where vmr_a >= 1e-6 rat.  O3 and N2O are so scarce (rat up to 6e5) that MLS water vapour does not get there: the first
            # species is raised to 3e-6 rat where that stays below 4 % (a tropical surface value); below that level band 7 cannot be capped
            lev = jp + 1 if r["kind"] == "jp1" else (jp if r["kind"] == "main" else np.full_like(jp, r["kind"]))
            need = 3.0e-6 * CHI[a][lev - 1] / CHI[b][lev - 1]
            vmr[a] = np.where(inreg & (need > vmr[a]) & (need <= 0.04), need, vmr[a])
            vmr[b] = np.where(inreg, 0.0, vmr[b])
        else:
            lev = jp if r["kind"] == "main" else (jp + 1 if r["kind"] == "jp1" else np.full_like(jp, r["kind"]))
            rat = CHI[a][lev - 1] / CHI[b][lev - 1]
            q = r["s"] / (1.0 - r["s"]) * rat                    # the ratio of the two amounts that gives specparm = s
            # the minority gas is scaled: whichever of the two has to come DOWN from its MLS value (so that no other gas threshold is crossed)
            down_a = q * vmr[b] <= vmr[a]
            va = np.where(down_a, q * vmr[b], vmr[a])
            with np.errstate(divide="ignore"):
                vb = np.where(down_a, vmr[b], vmr[a] / np.where(q > 0, q, 1.0))
            vmr[a], vmr[b] = np.where(inreg, va, vmr[a]), np.where(inreg, vb, vmr[b])
    elif r["type"] == "adj":
        ref = CHI[r["gas"]][jp] if r["ref"] is None else r["ref"]
        vmr[r["gas"]] = r["f"] * r["thr"] * ref * np.ones(nlay)
    elif r["type"] == "zero":
        vmr[r["gas"]] = np.zeros(nlay)
    return dict(plev=plev, play=play, tlay=tlay, tlev=tlev, tsfc=tlay[0] + 2.0, vmr=vmr)


def make_gas_states(nlay=52, seed=0, order="shuffled"):
    """The designed set as GCM-interface inputs (clear sky, icld = 0, idrv = 0; see with_clouds), plus
      labels   what every column was built for
      perm     column j of this dict is column perm[j] of the grouped order
    order "grouped": the columns of one stencil branch side by side, so that whole waves take one branch; "shuffled": a permutation
    seeded by `seed`, so that neighbouring lanes take different branches and different jp.  The permutation keeps the two replicas of
    every design point in different halves of the set, whose first half is a multiple of 64 columns: they never share a 64-column block.
    The seed also sets the emissivities; everything else is constructed."""
    base = sorted(_recipes(), key=_class)
    base += [dict(type="high", ps=ps) for ps in HIGH_PS[0::2]]
    second = list(base[:-3]) + [dict(type="high", ps=ps) for ps in HIGH_PS[1::2]]
    pad = (-len(base)) % 64
    fill = [dict(type="fill", psf=f) for f in np.linspace(0.55, 1.04, pad)]
    plan = [(r, *REPLICAS[0]) for r in base] + [(r, 1.0, (-4.0, 6.0)[n % 2]) for n, r in enumerate(fill)] + [(r, *REPLICAS[1]) for r in second]
    ncol, half = len(plan), len(base) + pad
    cols = [_column(nlay, r, psf, dt) for r, psf, dt in plan]
    rng = np.random.default_rng(seed)
    perm = np.arange(ncol) if order == "grouped" else np.concatenate([rng.permutation(half), half + rng.permutation(ncol - half)])
    if order not in ("grouped", "shuffled"):
        raise ValueError(order)
    if order == "shuffled":
        # column RAGGED_END - 1 is an extreme state (h2o/co2 capped at oneminus): a call of the first RAGGED_END columns ends its ragged
        # last window of 256 with it
        ext = next(j for j, (r, _, _) in enumerate(plan) if r["type"] == "spec" and r["s"] == CLAMP and r["kind"] == "main"
                   and (r["a"], r["b"], r["region"]) == (H2O, CO2, "lower"))
        at = int(np.nonzero(perm == ext)[0][0])
        perm[[at, RAGGED_END - 1]] = perm[[RAGGED_END - 1, at]]
    emis = 1.0 - 0.04 * np.random.default_rng(seed + 1).uniform(size=(ncol, 1)) * np.ones((1, NBND))
    st = lambda k: np.stack([c[k] for c in cols])
    d = dict(play=st("play"), plev=st("plev"), tlay=st("tlay"), tlev=st("tlev"), tsfc=np.array([c["tsfc"] for c in cols]), emis=emis)
    for m, k in VMR_KEY.items():
        d[k] = np.stack([c["vmr"][m] for c in cols])
    z = np.zeros((ncol, nlay))
    d.update(cfc11vmr=z + 2.6e-10, cfc12vmr=z + 5.0e-10, cfc22vmr=z + 1.5e-10, ccl4vmr=z + 1.0e-10)
    d.update(cldfr=z, cliqwp=z, cicewp=z, reliq=z + 10.0, reice=z + 30.0, tauaer=np.zeros((ncol, nlay, NBND)))
    out = {k: np.asfortranarray(v[perm]) for k, v in d.items()}
    out["taucld"] = np.zeros((NBND, ncol, nlay), order="F")
    out.update(ncol=ncol, nlay=nlay, inflglw=2, iceflglw=3, liqflglw=1, icld=0, idrv=0,
               labels=[_label(plan[j][0]) + " [psf %.2f dT %+.0f]" % plan[j][1:] for j in perm], perm=perm)
    return out


CLOUD_KEYS = ("cldfr", "cliqwp", "cicewp", "reliq", "reice", "taucld")


def with_clouds(d):
    """the cloud arrays of synth's "cloudy" configuration laid over the set (icld = 2)"""
    c = make_gcm_inputs(d["ncol"], d["nlay"], "cloudy", col0=7000)
    o = dict(d)
    o.update({k: c[k] for k in CLOUD_KEYS})
    o["icld"] = 2
    return o


def take(d, idx):
    """the columns idx (an index array or a slice) of the inputs d"""
    idx = np.arange(d["ncol"])[idx]
    o = dict(d)
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            o[k] = np.asfortranarray(v[:, idx] if k == "taucld" else v[idx])
    o["labels"] = [d["labels"][j] for j in idx]
    o["ncol"] = len(idx)
    return o


def span_columns(d, n=16):
    """n columns that span the ledger: one per kind of design point, chosen by label (deterministic)"""
    want = ("h2o/co2 lower main s=0.12493", "h2o/co2 lower jp1 s=0.8758", "o3/co2 upper main s=0.89", "h2o/o3 lower main s=clamp",
            "h2o/ch4 lower main s=0.0 ", "h2o/n2o lower main s=0.87507", "n2o/co2 lower main s=0.9375", "h2o/co2 upper main s=0.11",
            "co2 at 1.05 x threshold [", "n2o at 2.50 x threshold", "surface at 1085 hPa", "o3 = 0", "allupper grid", "dT = -70 K",
            "n2o/co2 lower ref1 s=0.6875", "h2o/n2o lower ref3 s=0.0625")
    picks = []
    for w in want[:n]:
        hit = [j for j, lab in enumerate(d["labels"]) if lab.startswith(w) or w in lab]
        assert hit, w
        picks.append(hit[0])
    return np.array(picks)


# ------------------------------------------------------------------------------------------------------------------ prepared columns
CO_DECADES = (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3)     # CO volume mixing ratio: six decades
WX_SCALES = (0.0, 0.1, 1.0, 10.0, 100.0)                     # of the four halocarbon amounts


def prepared_companion(d, inatm, n=48):
    """Prepared columns of n columns of the set (spread over it), with what the GCM interface cannot vary: the CO amount (wkl row 5)
    over six decades and the four cross-section amounts wx scaled, each halocarbon by its own factor."""
    idx = np.unique(np.linspace(0, d["ncol"] - 1, n).astype(int))
    cols = []
    for n_, i in enumerate(idx):
        c = inatm(d, int(i), 0)
        c["wkl"][4] = c["coldry"] * CO_DECADES[n_ % len(CO_DECADES)]
        c["wbrodl"] = c["wbrodl"] - c["wkl"][4]
        for m in range(4):
            c["wx"][m] = c["wx"][m] * WX_SCALES[(n_ + 2 * m) % len(WX_SCALES)]
        cols.append(c)
    return idx, cols
