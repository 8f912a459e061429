"""rrtmg_lw_hip_solve and rrtmg_lw_hip_solve_device (include/rrtmg_lw_hip.h, "The solver on the caller's optical depths and sources").

1. The numpy restatement (tests/solve_ref.py, pinned to the reference's Fortran on the CPU by tests/test_solve_ref.py) on the cloudy
   branches against the oracle: tau and odcld formed from the HIP gas optics, cloud_optics_ref and the oracle's generator.  Bound: the
   project's parity bars (README.md), 0.01 W m-2 and 0.001 K d-1 - the HIP taug differs from the oracle's at 1e-12, which can move a
   table index, so the tight bound does not apply here.
2. The entry against the restatement, same inputs bit for bit, on designed inputs that reach every branch (solve_ref.designed_inputs):
   cloud 0 / 1 / 2, idrv 0 / 1, host and device entry, one case in the 256-g-point library.  Bound: solve_ref.FTOL = 1e-9 W m-2 and
   heatfac * 2 * FTOL / |dp|.
3. The closed loop on the device - gas optics -> cloud optics -> cloud cover (submask) -> two torch expressions -> solve - against
   rrtmg_lw_device (icld 0, 1) and rrtmg_lw_mcica_subcol_device (same seed).  Bound: the parity bars; the production sweeps use float32
   transmittance tables.
4. The contract: EARG cases write nothing, NULL optional outputs, neighbour independence bit for bit (within a call and across column
   batches), host = device bit for bit, the device entry on a caller's stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import REFERENCE
from rrtmg_lw_amd.synth import make_gcm_inputs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_cover_ref as ccr  # noqa: E402
import cloud_optics_ref as cor  # noqa: E402
import cloud_states as cs  # noqa: E402
import solve_ref as sr  # noqa: E402
from test_cloud_state_coverage import subcolumns  # noqa: E402
from test_g256 import hip256  # noqa: E402,F401  (the fixture that selects the 256-g-point library for one test)
from test_hip_device_views import _dev, _host, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

PARITY_FLUX, PARITY_HR = 0.01, 0.001
FLUX = ("uflx", "dflx", "uflxc", "dflxc")
EARG = 2
FILL = -5.0
IN = ("plev", "emis", "tau", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt", "cldfr", "odcld", "submask")
OUT = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
SHAPES = [(70, 5), (130, 33)]          # each with a ragged last 64-column block; 130: more than one full block

_DESIGNED, _WANT = {}, {}


def designed(ncol, nlay, ng=140):
    if (ncol, nlay, ng) not in _DESIGNED:
        d = sr.designed_inputs(ncol, nlay, ng)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _DESIGNED[(ncol, nlay, ng)] = d
    return _DESIGNED[(ncol, nlay, ng)]


def want(oracle, ncol, nlay, cloud, ng=140):
    """Once per (shape, cloud): the restatement with idrv = 1 (the fluxes do not depend on idrv).  Shared and left unchanged."""
    key = (ncol, nlay, cloud, ng)
    if key not in _WANT:
        w = sr.solve(oracle.luts(), designed(ncol, nlay, ng), cloud=cloud, idrv=1)
        for k in OUT:
            w[k].setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def take(d, idx):
    """the columns idx of a solve call's inputs"""
    o = {k: (np.asfortranarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    o["ncol"] = len(np.arange(d["ncol"])[idx])
    return o


def device_call(hip, d, cloud, idrv, clear=True, fill=float("nan")):
    import torch
    ncol, nlay = d["ncol"], d["nlay"]
    xd = _dev({k: np.array(d[k], order="F").view(np.int32) if k == "submask" else np.array(d[k], order="F") for k in IN})
    xd.update(ncol=ncol, nlay=nlay)
    names = [k for k in OUT if (clear or not k.endswith("c")) and (idrv == 1 or not k.startswith("du"))]
    out = {k: torch.full((nlay if k.startswith("hr") else nlay + 1, ncol), fill, dtype=torch.float64, device="cuda:0").t() for k in names}
    s = _stream()
    hip.solve_device(xd, out, cloud=cloud, idrv=idrv, stream=s)
    hip.check(s)
    return _host(out)


def compare(got, w, plev, idrv, tag):
    """fluxes within FTOL, heating rates within the bound that goes with it; prints the observed maxima first"""
    keys = [k for k in OUT if k in got and (idrv == 1 or not k.startswith("du"))]
    ef = max(float(np.abs(got[k] - w[k]).max()) for k in keys if not k.startswith("hr"))
    eh = max(float((np.abs(got[k] - w[k]) / sr.hr_bound(plev)).max()) for k in keys if k.startswith("hr"))
    print(f"{tag}: max |d flux| = {ef:.3e} W m-2 (bound {sr.FTOL:.0e}), max |d hr| / bound = {eh:.3e}")
    for k in keys:
        assert np.isfinite(got[k]).all(), k
    assert ef <= sr.FTOL and eh <= 1.0, tag


# ---- 1. the restatement against the oracle, cloudy branches ------------------------------------------------------------------------------
def _optics(hip, d):
    """tau, fracs, the Planck terms from the HIP gas optics, the secants from cloud_optics_ref"""
    g = hip.gas_optics(d, idrv=1)
    sec = cor.secdiff(d)
    band = sr.bands(140)
    tau = sec[:, None, band] * (g["taug"] + np.asarray(d["tauaer"])[:, :, band])
    x = dict(ncol=d["ncol"], nlay=d["nlay"], plev=np.asarray(d["plev"]), emis=np.asarray(d["emis"]), tau=tau, fracs=g["fracs"])
    x.update({k: g[k] for k in ("planklay", "planklev", "plankbnd", "dplankbnd_dt")})
    return x, sec


def _cloudy_calls():
    return {"gcm-cloudy": make_gcm_inputs(70, 33, "cloudy", col0=5), "states-B211": cs.take(cs.family_b()[(2, 1, 1)], slice(30, 75)),
            "states-A31": cs.take(cs.family_a()[(3, 1)], slice(0, 40))}


@pytest.mark.parametrize("name", ("gcm-cloudy", "states-B211", "states-A31"))
def test_restatement_matches_the_oracle_on_cloudy_columns(hip, oracle, name):
    d = _cloudy_calls()[name]
    ncol, nlay = d["ncol"], d["nlay"]
    x, sec = _optics(hip, d)
    # rtrn: the secant of the CLOUD band
    x1 = dict(x, cldfr=np.asarray(d["cldfr"]), odcld=cor.cloud_band_secdiff(sec, cor.ncbands(d))[:, None, :] * cor.taucloud(d, 0))
    got = sr.solve(oracle.luts(), x1, cloud=1, idrv=1)
    ref = oracle.rrtmg_lw(ncol, nlay, 1, 1, d)
    ef = max(float(np.abs(got[k] - ref[k]).max()) for k in FLUX + ("duflx_dt", "duflxc_dt"))
    eh = max(float(np.abs(got[k] - ref[k]).max()) for k in ("hr", "hrc"))
    print(f"{name} rtrn: max |d flux| = {ef:.3e} W m-2, max |d hr| = {eh:.3e} K/d; cloudy cells {got['branches']}")
    assert got["branches"]["cloudy_table"] > 0 and ef <= PARITY_FLUX and eh <= PARITY_HR
    # rtrnmc on the oracle generator's sub-columns
    dd = subcolumns(oracle, d, 2)
    x2 = dict(x, submask=ccr.submask(dd["cldfmcl"]), odcld=sec[:, None, :] * cor.taucloud(d, 1))
    got = sr.solve(oracle.luts(), x2, cloud=2, idrv=1)
    ref = oracle.rrtmg_lw(ncol, nlay, 2, 1, dd, mcica=True)
    ef = max(float(np.abs(got[k] - ref[k]).max()) for k in FLUX + ("duflx_dt", "duflxc_dt"))
    eh = max(float(np.abs(got[k] - ref[k]).max()) for k in ("hr", "hrc"))
    print(f"{name} rtrnmc: max |d flux| = {ef:.3e} W m-2, max |d hr| = {eh:.3e} K/d")
    assert got["branches"]["cloudy_table"] > 0 and ef <= PARITY_FLUX and eh <= PARITY_HR


# ---- 2. the entry against the restatement ------------------------------------------------------------------------------------------------
def test_designed_inputs_reach_every_branch(oracle):
    for ncol, nlay in SHAPES:
        d = designed(ncol, nlay)
        for cloud in (1, 2):
            b = want(oracle, ncol, nlay, cloud)["branches"]
            assert all(b[k] > 0 for k in sr.BRANCHES), (ncol, nlay, cloud, b)
        assert (d["emis"] < 1).all() and (d["tau"] == 0.06).any() and (d["tau"] < 0).any()
        cf = d["cldfr"]
        assert ((cf > 0) & (cf < 1e-6)).any() and (cf == 1e-6).any() and (cf[:, -1] >= 1e-6).any() and (cf[:, 0] >= 1e-6).any() and (~cf.any(axis=1)).any()
        bits = sr.unpack_mask(d["submask"], 140)
        assert (bits.sum(axis=2) == 1).any() and bits.all(axis=2).any() and (~bits.any(axis=(1, 2))).any()
        assert ((d["submask"][:, :, -1] >> np.uint32(12)) != 0).any()               # bits above NG are set somewhere


@pytest.mark.parametrize("idrv", (0, 1))
@pytest.mark.parametrize("cloud", (0, 1, 2))
@pytest.mark.parametrize("ncol,nlay", SHAPES)
def test_entries_match_the_restatement(hip, oracle, ncol, nlay, cloud, idrv):
    d, w = designed(ncol, nlay), want(oracle, ncol, nlay, cloud)
    host = hip.solve(dict(d), cloud=cloud, idrv=idrv)
    compare(host, w, d["plev"], idrv, f"host {ncol}x{nlay} cloud {cloud} idrv {idrv}")
    dev = device_call(hip, d, cloud, idrv)
    compare(dev, w, d["plev"], idrv, f"device {ncol}x{nlay} cloud {cloud} idrv {idrv}")
    for k in dev:
        assert np.array_equal(dev[k], host[k]), k                                   # host and device entry agree bit for bit
    if cloud == 0:
        assert np.array_equal(host["uflx"], host["uflxc"]) and np.array_equal(host["dflx"], host["dflxc"]) and np.array_equal(host["hr"], host["hrc"])


def test_g256_library(hip256, oracle):
    ncol, nlay = 70, 5
    assert hip256.gpoints() == 256 and hip256.mask_words() == 8
    d, w = designed(ncol, nlay, 256), want(oracle, ncol, nlay, 2, 256)
    assert d["submask"].shape == (ncol, nlay, 8)
    compare(hip256.solve(dict(d), cloud=2, idrv=1), w, d["plev"], 1, "g256 host cloud 2")
    compare(device_call(hip256, d, 1, 1), want(oracle, ncol, nlay, 1, 256), d["plev"], 1, "g256 device cloud 1")


# ---- 3. the closed loop on the device ----------------------------------------------------------------------------------------------------
def _closed_loop(hip, d, cloud, seed=None):
    """gas optics -> cloud optics -> (submask) -> tau, odcld -> solve, all on the device; d: torch inputs of rrtmg_lw_device"""
    import torch
    ncol, nlay, ng = d["ncol"], d["nlay"], hip.gpoints()
    s = _stream()
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda:0")
    g = dict(taug=f64(ng, nlay, ncol), fracs=f64(ng, nlay, ncol), planklay=f64(16, nlay, ncol), planklev=f64(16, nlay + 1, ncol),
             plankbnd=f64(16, ncol), dplankbnd_dt=f64(16, ncol))
    hip.gas_optics_device(d, g, stream=s, idrv=1)
    co = arrays.empty_like_form(["taucloud", "secdiff"], ncol, nlay, REFERENCE, device="cuda:0", fill=0.0)
    co["ncbands"] = torch.zeros(ncol, dtype=torch.int32, device="cuda:0")
    hip.cloud_optics_device(d, co, imca=1 if cloud == 2 else 0, stream=s)
    x = dict(ncol=ncol, nlay=nlay, plev=d["plev"], emis=d["emis"], cldfr=d["cldfr"])
    x.update({k: v.permute(*reversed(range(v.dim()))) for k, v in g.items() if k not in ("taug",)})
    band = torch.as_tensor(sr.bands(ng), device="cuda:0")
    sec = co["secdiff"]
    # the two lines a host writes: the clear-sky and the cloud optical depth along the diffusivity path
    x["tau"] = (sec[:, band][:, None, :] * (g["taug"].permute(2, 1, 0) + d["tauaer"][:, :, band])).permute(2, 1, 0).contiguous().permute(2, 1, 0)
    if cloud == 2:
        seccld = sec
        m = torch.zeros(hip.mask_words(), nlay, ncol, dtype=torch.int32, device="cuda:0").permute(2, 1, 0)
        hip.mcica_cloud_cover_device(dict(ncol=ncol, nlay=nlay, play=d["play"], cldfr=d["cldfr"]), {"submask": m}, 2, seed, irng=0, stream=s)
        x["submask"] = m
    else:
        icb = torch.as_tensor(np.stack([cor.icb(n) - 1 for n in (1, 5, 16)]).astype(np.int64), device="cuda:0")             # ipat, 0-based
        row = torch.searchsorted(torch.tensor([1, 5, 16], dtype=torch.int32, device="cuda:0"), co["ncbands"])
        seccld = torch.gather(sec, 1, icb[row])
    x["odcld"] = (seccld[:, None, :] * co["taucloud"]).permute(2, 1, 0).contiguous().permute(2, 1, 0)
    out = {k: torch.full((nlay if k.startswith("hr") else nlay + 1, ncol), float("nan"), dtype=torch.float64, device="cuda:0").t() for k in OUT}
    hip.solve_device(x, out, cloud=cloud, idrv=1, stream=s)
    hip.check(s)
    return _host(out)


@pytest.mark.parametrize("kind", ("icld0", "icld1", "mcica"))
def test_closed_loop_matches_the_production_entries(hip, kind):
    import torch
    ncol, nlay = 130, 33
    dn = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=9)
    d = _dev(dn)
    ref = {k: torch.full((nlay if k.startswith("hr") else nlay + 1, ncol), float("nan"), dtype=torch.float64, device="cuda:0").t() for k in OUT}
    s = _stream()
    if kind == "mcica":
        hip.rrtmg_lw_mcica_subcol_device(d, ref, 77, 0, icld=2, idrv=1, stream=s)
        got = _closed_loop(hip, d, 2, seed=77)
    else:
        icld = int(kind[-1])
        hip.rrtmg_lw_device(d, ref, icld=icld, idrv=1, stream=s)
        got = _closed_loop(hip, d, icld)
    hip.check(s)
    ref = _host(ref)
    ef = max(float(np.abs(got[k] - ref[k]).max()) for k in FLUX + ("duflx_dt", "duflxc_dt"))
    eh = max(float(np.abs(got[k] - ref[k]).max()) for k in ("hr", "hrc"))
    print(f"closed loop {kind}: max |d flux| = {ef:.3e} W m-2, max |d hr| = {eh:.3e} K/d")
    assert ef <= PARITY_FLUX and eh <= PARITY_HR
    if kind != "icld0":
        assert np.abs(got["uflx"] - got["uflxc"]).max() > 1.0            # the columns are cloudy


# ---- 4. the contract ---------------------------------------------------------------------------------------------------------------------
def _raw(hip, d, cloud, idrv, ins, outs, **kw):
    null = C.c_void_p(0)
    p = lambda a: null if a is None else C.c_void_p(a.ctypes.data)
    rc = hip.lib().rrtmg_lw_hip_solve(C.c_int(kw.get("ncol", d["ncol"])), C.c_int(kw.get("nlay", d["nlay"])), C.c_int(cloud), C.c_int(idrv),
                                      *[p(ins.get(k)) for k in IN], *[p(outs.get(k)) for k in OUT])
    return rc, hip.lib().rrtmg_lw_hip_last_error().decode()


def test_argument_errors_name_the_argument_and_write_nothing(hip):
    ncol, nlay = 70, 5
    d = designed(ncol, nlay)
    ins = {k: np.array(d[k], order="F") for k in IN}
    fresh = lambda: {k: np.full((ncol, nlay if k.startswith("hr") else nlay + 1), FILL, order="F") for k in OUT}
    cases = [
        (dict(cloud=3), "cloud"), (dict(cloud=-1), "cloud"), (dict(idrv=2), "idrv"),
        (dict(drop_in="tau"), "tau"), (dict(drop_in="plev"), "plev"), (dict(drop_in="cldfr", cloud=1), "cldfr"), (dict(drop_in="odcld", cloud=2), "odcld"),
        (dict(drop_in="submask", cloud=2), "submask"), (dict(drop_in="dplankbnd_dt", idrv=1), "dplankbnd_dt"),
        (dict(drop_out="hr"), "hr"), (dict(drop_out="duflxc_dt", idrv=1), "duflxc_dt"), (dict(drop_out="dflxc"), "dflxc"), (dict(drop_out="hrc"), "hrc"),
        (dict(ncol=0), "ncol"), (dict(nlay=604), "nlay"),
    ]
    for spec, word in cases:
        i, o = dict(ins), fresh()
        if "drop_in" in spec:
            i[spec["drop_in"]] = None
        if "drop_out" in spec:
            o[spec["drop_out"]] = None
        kw = {k: spec[k] for k in ("ncol", "nlay") if k in spec}
        rc, text = _raw(hip, d, spec.get("cloud", 2), spec.get("idrv", 1), i, o, **kw)
        assert rc == EARG and word in text, (spec, rc, text)
        assert all((v == FILL).all() for v in o.values() if v is not None), spec
    # an output that shares a byte with an input, or with another output
    o = fresh()
    o["hr"] = ins["cldfr"]
    keep = ins["cldfr"].copy()
    rc, text = _raw(hip, d, 1, 0, ins, o)
    assert rc == EARG and "hr" in text and "cldfr" in text and np.array_equal(ins["cldfr"], keep), text
    o = fresh()
    buf = np.full(2 * ncol * (nlay + 1) - 1, FILL)
    o["uflx"], o["dflx"] = buf[:ncol * (nlay + 1)], buf[ncol * (nlay + 1) - 1:]
    rc, text = _raw(hip, d, 0, 0, ins, o)
    assert rc == EARG and "uflx" in text and "dflx" in text and (buf == FILL).all(), text
    # an input the call does not read may overlap: cloud = 0 never reads cldfr
    o = fresh()
    o["hr"] = np.array(ins["cldfr"], order="F")
    rc, text = _raw(hip, d, 0, 0, dict(ins, cldfr=o["hr"]), o)
    assert rc == 0, text


def test_null_optional_outputs_are_left_alone(hip, oracle):
    ncol, nlay = 70, 5
    d = designed(ncol, nlay)
    full = hip.solve(dict(d), cloud=1, idrv=1)
    part = hip.solve(dict(d), cloud=1, idrv=0, out={"uflxc": None, "dflxc": None, "hrc": None})
    assert part["uflxc"] is None and "duflx_dt" not in part
    for k in ("uflx", "dflx", "hr"):
        assert np.array_equal(part[k], full[k]), k
    dev = device_call(hip, d, 1, 0, clear=False)
    assert set(dev) == {"uflx", "dflx", "hr"} and all(np.array_equal(dev[k], full[k]) for k in dev)
    # idrv = 0 does not touch the derivative arrays it is handed
    ins = {k: np.array(d[k], order="F") for k in IN}
    o = {k: np.full((ncol, nlay if k.startswith("hr") else nlay + 1), FILL, order="F") for k in OUT}
    rc, text = _raw(hip, d, 1, 0, ins, o)
    assert rc == 0 and (o["duflx_dt"] == FILL).all() and (o["duflxc_dt"] == FILL).all() and np.array_equal(o["uflx"], full["uflx"]), text


@pytest.mark.parametrize("cloud", (1, 2))
def test_a_column_does_not_depend_on_its_neighbours(hip, cloud):
    ncol, nlay = 130, 33
    d = designed(ncol, nlay)
    tail = take(d, slice(64, 130))
    assert tail["ncol"] == 66
    whole, alone = device_call(hip, d, cloud, 1), device_call(hip, tail, cloud, 1)
    for k in OUT:
        assert np.array_equal(whole[k][64:], alone[k]), k
    try:
        hip.set_batch(64)                                   # the call now spans three column batches
        assert hip.effective_batch(nlay) == 64
        dev, host = device_call(hip, d, cloud, 1), hip.solve(dict(d), cloud=cloud, idrv=1)
    finally:
        hip.set_batch(0)
    for k in OUT:
        assert np.array_equal(dev[k], whole[k]) and np.array_equal(host[k], whole[k]), k


def test_device_entry_runs_on_the_callers_stream(hip):
    import torch
    ncol, nlay = 70, 5
    d = designed(ncol, nlay)
    want_ = device_call(hip, d, 2, 1)
    xd = _dev({k: np.array(d[k], order="F").view(np.int32) if k == "submask" else np.array(d[k], order="F") for k in IN})
    xd.update(ncol=ncol, nlay=nlay)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = {k: torch.full((nlay if k.startswith("hr") else nlay + 1, ncol), float("nan"), dtype=torch.float64, device="cuda:0").t() for k in OUT}
        hip.solve_device(xd, out, cloud=2, idrv=1, stream=side.cuda_stream)
        hip.check(side.cuda_stream)                          # errors and completion come through check(stream)
    got = _host(out)
    assert all(np.array_equal(got[k], want_[k]) for k in OUT)
    with pytest.raises(hip.RrtmgLwError, match="cloud"):
        hip.solve_device(xd, out, cloud=5, idrv=1, stream=side.cuda_stream)
    with pytest.raises((TypeError, ValueError)):
        hip.solve_device(dict(xd, tau=xd["tau"].float()), out, cloud=2, idrv=1)
    with pytest.raises(ValueError):
        hip.solve_device(dict(xd, fracs=xd["fracs"].contiguous()), out, cloud=2, idrv=1)


def test_a_non_finite_input_stays_in_its_column(hip):
    ncol, nlay = 70, 5
    d = designed(ncol, nlay)
    good = device_call(hip, d, 1, 1)
    tau = np.array(d["tau"], order="F")
    tau[3, 2, 7], tau[5, 1, 100], tau[69, 4, 139] = np.nan, np.inf, np.nan
    bad = device_call(hip, dict(d, tau=tau), 1, 1)
    hit = np.zeros(ncol, dtype=bool)
    hit[[3, 5, 69]] = True
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
        assert not np.isfinite(bad[k][hit]).all(axis=1).any(), k
        assert np.array_equal(bad[k][~hit], good[k][~hit]), k
