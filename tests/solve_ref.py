"""What rrtmg_lw_hip_solve* must return, from the recurrences in include/rrtmg_lw_hip.h ("The solver on the caller's optical depths and
sources"): a numpy restatement of rtrn's / rtrnmc's level loops (src/rrtmg_lw_rtrn.f90:361-604), vectorised over the columns, looping
over g-points and levels.  Every operation is a float64 numpy operation that rounds on its own, in the reference's order; the tables
come from the oracle (Oracle.luts()), delwave and the band of each g-point from lw_static.bin.  It also counts, per call, how many cells
took each branch (`branches`), so that a test can require that its inputs reach them all.  A helper module (not a conftest) for
tests/test_solve_ref.py, which pins it to the reference's Fortran, and the GPU tests of the entry.  No GPU, no library."""
import os

import numpy as np

from rrtmg_lw_amd.blob import read_blob

NBND = 16
STATIC = read_blob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rrtmg_lw_amd", "data", "lw_static.bin"))
DELWAVE = np.asarray(STATIC["delwave"], dtype=np.float64)
FTOL = 1e-9                       # W m-2: fluxes below 700 W m-2, a few hundred rounded operations per g-point -> a few 1e-11; x 30
HEATFAC = 9.8066 * 8.6400e4 / (1004.0 * 1.e2)
FLUXFAC = (2.0 * np.arcsin(1.0)) * 2.e4
BPADE = 1.0 / 0.278
REC_6 = 0.166667
WTDIFF = 0.5
BRANCHES = ("clear_series", "clear_table", "cloudy_thin_total", "cloudy_thin_gas", "cloudy_table", "negative_tau", "index_10000")


def bands(ng):
    """0-based band of every g-point"""
    return np.repeat(np.arange(NBND), STATIC["ngc"] if ng == 140 else np.full(NBND, 16))


def hr_bound(plev):
    """the heating-rate bound that goes with FTOL: two net fluxes of two fluxes each"""
    plev = np.asarray(plev)
    return HEATFAC * 2 * FTOL / np.abs(plev[:, :-1] - plev[:, 1:])


def interp_planck(tab, t):
    """setcoef :173-269: tab (181, 16) at temperatures t (...) -> (..., 16)"""
    x = np.asarray(t, dtype=np.float64) - 159.0
    ind = np.clip(np.trunc(x).astype(int), 1, 180)
    f = (x - ind)[..., None]
    return tab[ind - 1] + f * (tab[ind] - tab[ind - 1])


def planck(tlay, tlev, tsfc, emis):
    """setcoef's Planck integrals: planklay (ncol,nlay,16), planklev (ncol,nlay+1,16), plankbnd, dplankbnd_dt (ncol,16)"""
    tp, td = STATIC["totplnk"].reshape(181, 16), STATIC["totplnkderiv"].reshape(181, 16)
    emis = np.asarray(emis)
    return dict(planklay=interp_planck(tp, tlay), planklev=interp_planck(tp, tlev), plankbnd=emis * interp_planck(tp, tsfc),
                dplankbnd_dt=emis * interp_planck(td, tsfc))


def unpack_mask(submask, ng):
    """(ncol, nlay, ng) bool from the (ncol, nlay, MW) uint32 words; bits at and above ng are ignored"""
    m = np.asarray(submask).astype(np.uint32)
    return np.stack([(m[:, :, g // 32] >> np.uint32(g % 32)) & np.uint32(1) for g in range(ng)], axis=2).astype(bool)


def _index(od):
    with np.errstate(invalid="ignore"):
        x = 1e4 * (od / (BPADE + od)) + 0.5
    return np.clip(np.where(np.isfinite(x), x, 0.0), 0, 10000).astype(int)


def _cell(luts, cldy, od, odc, f, blay, dup, ddn, count):
    """one level of one g-point for all columns: atrans, atot, bbd, bbdtot, bbu, bbutot, gassrc_down (what rtrn forms of a cell)"""
    tau_tbl, exp_tbl, tfn_tbl = luts
    with np.errstate(invalid="ignore", over="ignore"):
        poison = (od - od) + (odc - odc)
        count["negative_tau"] += int((od < 0.0).sum())
        od = np.where(od < 0.0, 0.0, od)
        series = od - 0.5 * od * od
        odtot = od + odc
        thin_tot, thin_gas = cldy & (odtot < 0.06), od <= 0.06
        case2 = cldy & ~thin_tot & thin_gas
        case3 = cldy & ~thin_tot & ~thin_gas
        i = _index(od)
        atrans = np.where(thin_gas, series, 1. - exp_tbl[i])
        t = np.where(thin_gas, REC_6 * od, tfn_tbl[i])
        od3 = tau_tbl[i]
        odtot = np.where(case3, od3 + odc, odtot)
        j = _index(odtot)
        atot = np.where(thin_tot, odtot - 0.5 * odtot * odtot, 1. - exp_tbl[j])
        tt = np.where(thin_tot, REC_6 * odtot, tfn_tbl[j])
        bbd = f * (blay + ddn * t)
        bbu = f * (blay + dup * t)
        bbdtot = f * (blay + ddn * tt)
        bbutot = f * (blay + dup * tt)
        gassrc = np.where(case3, atrans * f * (blay + t * ddn), bbd * atrans)
        count["clear_series"] += int((~cldy & thin_gas).sum())
        count["clear_table"] += int((~cldy & ~thin_gas).sum())
        count["cloudy_thin_total"] += int(thin_tot.sum())
        count["cloudy_thin_gas"] += int(case2.sum())
        count["cloudy_table"] += int(case3.sum())
        count["index_10000"] += int(((~thin_gas) & (i == 10000)).sum())
        atrans = np.where(poison != 0.0, poison, atrans)
    return atrans, atot, bbd, bbdtot, bbu, bbutot, gassrc


def solve(luts, d, cloud=0, idrv=0, heatfac=HEATFAC):
    """dict of uflx, dflx, uflxc, dflxc, duflx_dt, duflxc_dt (ncol, nlay+1), hr, hrc (ncol, nlay), branches (dict of counts).
    luts = Oracle.luts(): (tau_tbl, exp_tbl, tfn_tbl).  d: the arrays of rrtmg_lw_hip_solve by name."""
    tau, fracs = np.asarray(d["tau"], dtype=np.float64), np.asarray(d["fracs"], dtype=np.float64)
    ncol, nlay, ng = tau.shape
    band = bands(ng)
    planklay, planklev = np.asarray(d["planklay"]), np.asarray(d["planklev"])
    plankbnd, emis, plev = np.asarray(d["plankbnd"]), np.asarray(d["emis"]), np.asarray(d["plev"])
    dpl = np.asarray(d["dplankbnd_dt"]) if idrv == 1 else np.zeros((ncol, NBND))
    count = {k: 0 for k in BRANCHES}
    if cloud == 0:
        cldy = np.zeros((ncol, nlay), dtype=bool)
    elif cloud == 1:
        cldfr = np.asarray(d["cldfr"])
        cldy = cldfr >= 1.e-6
    else:
        bits = unpack_mask(d["submask"], ng)
        cldy = bits.any(axis=2)
    odcld = np.asarray(d["odcld"]) if cloud else None
    acc = {k: np.zeros((ncol, nlay + 1, NBND)) for k in ("u", "d", "uc", "dc", "du", "duc")}
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(ng):
            b = band[g]

            def terms(k):
                blay = planklay[:, k, b]
                if cloud == 0:
                    cf = odc = efc = np.zeros(ncol)
                else:
                    on = cldy[:, k] if cloud == 1 else bits[:, k, g]
                    cf = np.where(on, cldfr[:, k] if cloud == 1 else 1.0, 0.0)
                    odc = np.where(on, odcld[:, k, b], 0.0)
                    efc = np.where(on, (1. - np.exp(-odc)) * cf, 0.0)
                c = _cell(luts, cldy[:, k], tau[:, k, g], odc, fracs[:, k, g], blay, planklev[:, k + 1, b] - blay, planklev[:, k, b] - blay, count)
                return cf, efc, c

            radld, radclrd = np.zeros(ncol), np.zeros(ncol)
            iclddn = np.zeros(ncol, dtype=bool)
            for lev in range(nlay, 0, -1):
                k = lev - 1
                cf, efc, (atrans, atot, bbd, bbdtot, bbu, bbutot, gassrc) = terms(k)
                cl = cldy[:, k]
                iclddn = iclddn | cl
                radld = np.where(cl, radld - radld * (atrans + efc * (1. - atrans)) + gassrc + cf * (bbdtot * atot - gassrc),
                                 radld + (bbd - radld) * atrans)
                acc["d"][:, k, b] += radld
                radclrd = np.where(iclddn, radclrd + (bbd - radclrd) * atrans, radld)
                acc["dc"][:, k, b] += radclrd
            rad0 = fracs[:, 0, g] * plankbnd[:, b]
            reflect = 1. - emis[:, b]
            radlu, radclru = rad0 + reflect * radld, rad0 + reflect * radclrd
            dlu = fracs[:, 0, g] * dpl[:, b]
            dclru = dlu
            acc["u"][:, 0, b] += radlu
            acc["uc"][:, 0, b] += radclru
            acc["du"][:, 0, b] += dlu
            acc["duc"][:, 0, b] += dclru
            for lev in range(1, nlay + 1):
                k = lev - 1
                cf, efc, (atrans, atot, bbd, bbdtot, bbu, bbutot, _) = terms(k)
                cl = cldy[:, k]
                gassrc = bbu * atrans
                radlu = np.where(cl, radlu - radlu * (atrans + efc * (1. - atrans)) + gassrc + cf * (bbutot * atot - gassrc),
                                 radlu + (bbu - radlu) * atrans)
                dlu = np.where(cl, dlu * cf * (1.0 - atot) + dlu * (1.0 - cf) * (1.0 - atrans), dlu * (1.0 - atrans))
                radclru = np.where(iclddn, radclru + (bbu - radclru) * atrans, radlu)
                dclru = np.where(iclddn, dclru * (1.0 - atrans), dlu)
                acc["u"][:, lev, b] += radlu
                acc["uc"][:, lev, b] += radclru
                acc["du"][:, lev, b] += dlu
                acc["duc"][:, lev, b] += dclru
        out = {}
        for k, name in (("u", "uflx"), ("d", "dflx"), ("uc", "uflxc"), ("dc", "dflxc")):
            tot = np.zeros((ncol, nlay + 1))
            for b in range(NBND):
                tot = tot + (acc[k][:, :, b] * WTDIFF) * DELWAVE[b]
            out[name] = np.asfortranarray(tot * FLUXFAC)
        for k, name in (("du", "duflx_dt"), ("duc", "duflxc_dt")):
            tot = np.zeros((ncol, nlay + 1))
            for b in range(NBND):
                tot = tot + (acc[k][:, :, b] * WTDIFF) * DELWAVE[b] * FLUXFAC
            out[name] = np.asfortranarray(tot)
        dp = plev[:, :-1] - plev[:, 1:]
        net, netc = out["uflx"] - out["dflx"], out["uflxc"] - out["dflxc"]
        out["hr"] = np.asfortranarray(heatfac * (net[:, :-1] - net[:, 1:]) / dp)
        out["hrc"] = np.asfortranarray(heatfac * (netc[:, :-1] - netc[:, 1:]) / dp)
    # every cell is visited twice (down and up): report cells, not visits
    out["branches"] = {k: v // 2 for k, v in count.items()}
    return out


def designed_inputs(ncol, nlay, ng, seed=11):
    """Inputs of rrtmg_lw_hip_solve that need no physics and reach every branch: tau log-uniform in 1e-7 .. 1e3 with some values negative,
    some exactly 0.06 and some huge (table position 10000); odcld small, medium and large, so that a cloudy cell meets odtot < 0.06,
    odepth <= 0.06 <= odtot and odepth > 0.06; cldfr straddling 1e-6; cloud in the top layer, in the bottom layer and in none; masks
    that are all zero, all one (with the bits above ng set too: they are ignored) and one set bit in an otherwise empty layer;
    emis < 1.  The Planck integrals are setcoef's at random temperatures, so that the fluxes have physical size (FTOL's derivation).
    Everything Fortran-ordered, as the entry takes it."""
    rng = np.random.default_rng(seed)
    mw = (ng + 31) // 32
    band = bands(ng)
    F = np.asfortranarray
    edges = np.linspace(0.0, 1.0, nlay + 1)
    plev = rng.uniform(950.0, 1040.0, ncol)[:, None] * (1.0 - edges[None, :]) ** 2 + 0.5 + rng.uniform(0.0, 0.01, (ncol, nlay + 1))
    assert (np.diff(plev, axis=1) < 0).all()
    tlev = rng.uniform(190.0, 310.0, (ncol, nlay + 1))
    tlay = 0.5 * (tlev[:, :-1] + tlev[:, 1:]) + rng.uniform(-3.0, 3.0, (ncol, nlay))
    emis = rng.uniform(0.6, 0.99, (ncol, NBND))
    d = dict(ncol=ncol, nlay=nlay, plev=F(plev), emis=F(emis))
    d.update({k: F(v) for k, v in planck(tlay, tlev, tlev[:, 0] + rng.uniform(-5.0, 5.0, ncol), emis).items()})
    tau = 10.0 ** rng.uniform(-7.0, 3.0, (ncol, nlay, ng))
    pick = rng.uniform(size=tau.shape)
    tau = np.where(pick < 0.02, -tau, tau)
    tau = np.where((pick >= 0.02) & (pick < 0.04), 0.06, tau)
    tau = np.where((pick >= 0.04) & (pick < 0.05), 1e9, tau)
    d["tau"] = F(tau)
    fr = rng.uniform(0.1, 1.0, (ncol, nlay, ng))
    bsum = np.zeros((ncol, nlay, NBND))
    for g in range(ng):
        bsum[:, :, band[g]] += fr[:, :, g]
    d["fracs"] = F(fr / bsum[:, :, band])
    kind = rng.integers(0, 3, (ncol, nlay, NBND))
    d["odcld"] = F(np.where(kind == 0, 10.0 ** rng.uniform(-5.0, -2.5, kind.shape), np.where(kind == 1, rng.uniform(0.05, 0.2, kind.shape), rng.uniform(1.0, 8.0, kind.shape))))
    values = np.array([0.0, 0.0, 0.0, 5e-7, 9.999e-7, 1e-6, 2e-6, 0.3, 0.75, 1.0])
    cldfr = values[rng.integers(0, len(values), (ncol, nlay))]
    col = np.arange(ncol)
    cldfr[col % 4 == 0] = 0.0                               # no cloud
    cldfr[col % 4 == 1, nlay - 1] = 0.4                     # cloud in the top layer
    cldfr[col % 4 == 2, 0] = 0.6                            # ... in the bottom layer
    d["cldfr"] = F(cldfr)
    bits = rng.uniform(size=(ncol, nlay, ng)) < np.where(cldfr >= 1e-6, np.maximum(cldfr, 0.3), 0.0)[:, :, None]
    m = np.zeros((ncol, nlay, mw), dtype=np.uint32)
    for g in range(ng):
        m[:, :, g // 32] |= bits[:, :, g].astype(np.uint32) << np.uint32(g % 32)
    lay = np.arange(nlay)
    m[np.ix_(col % 8 == 3, lay % 3 == 0)] = np.uint32(0xFFFFFFFF)           # all ones, the bits above ng too
    m[np.ix_(col % 8 == 5, lay % 2 == 1)] = 0                               # one set bit in an otherwise empty layer
    m[np.ix_(col % 8 == 5, lay % 2 == 1, [(ng - 1) // 32])] = np.uint32(1) << np.uint32((ng - 1) % 32)
    if ng % 32:
        m[np.ix_(col % 8 == 6, lay % 2 == 0)] = 0                           # only bits above ng: an empty layer
        m[np.ix_(col % 8 == 6, lay % 2 == 0, [mw - 1])] = np.uint32(0xFFFFFFFF) << np.uint32(ng % 32)
    m[col % 8 == 7] = 0                                                     # no cloud
    d["submask"] = F(m)
    return d
