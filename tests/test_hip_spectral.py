"""Spectral (per-band) fluxes of the GCM entries (include/rrtmg_lw_hip.h, "Spectral (per-band) fluxes"): the broadband outputs of the
*_spectral entries equal the plain entries' bit for bit, the band fluxes add up to the broadband ones, each band equals the oracle's
column driver for that band (band 16 in the broadband call's convention), and every (band, level, stream) is written on every path.
Every spectral output is prefilled with NaN, so that a value nobody wrote fails."""
import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

BROAD = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
SPEC = ("uflxs", "dflxs", "uflxcs", "dflxcs")
PAIRS = (("uflxs", "uflx"), ("dflxs", "dflx"), ("uflxcs", "uflxc"), ("dflxcs", "dflxc"))
SUM_TOL = 1e-9       # W m-2: the bands of a level add up to the broadband flux (rounding only)
BAND_TOL = 5e-5      # W m-2: against the oracle (tests/test_hip_parity.py: TIGHT_FLUX)


def _nan_out(ncol, nlay, idrv=0, clear=True):
    f = lambda *s: np.full(s, np.nan, order="F")
    out = {k: f(ncol, nlay + 1) for k in ("uflx", "dflx", "uflxc", "dflxc")}
    out.update(hr=f(ncol, nlay), hrc=f(ncol, nlay))
    if idrv == 1:
        out.update(duflx_dt=f(ncol, nlay + 1), duflxc_dt=f(ncol, nlay + 1))
    for k in SPEC:
        out[k] = f(ncol, nlay + 1, 16) if clear or k in ("uflxs", "dflxs") else None
    return out


def _spec_only(ncol, nlay):
    return {k: np.full((ncol, nlay + 1, 16), np.nan, order="F") for k in SPEC}


def _check_sums(got, tag=""):
    for s, b in PAIRS:
        assert np.isfinite(got[s]).all(), (tag, s, "values left unwritten")
        err = np.abs(got[s].sum(axis=2) - got[b]).max()
        assert err <= SUM_TOL, (tag, s, err)


# ------------------------------------------------------------------------------------------------------------ 1. broadband untouched
def _with_subcolumns(oracle, d, icld, seed=140):
    sc = oracle.mcica_subcol(d["ncol"], d["nlay"], icld, seed, 0, d["play"], d["cldfr"], d["cicewp"], d["cliqwp"], d["reice"],
                             d["reliq"], d["taucld"], np.zeros((d["ncol"], d["nlay"])))
    dd = dict(d)
    dd.update({k: sc[k] for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "taucmcl")})
    return dd


@pytest.mark.parametrize("case", ["nomcica icld0", "nomcica icld1", "nomcica icld2", "aer_idrv", "mcica arrays", "fused kissvec",
                                  "fused mersenne"])
def test_broadband_outputs_are_untouched(hip, oracle, case):
    ncol, nlay = 300, 60
    config = "aer_idrv" if case == "aer_idrv" else ("clear" if case.endswith("icld0") else "cloudy")
    d = make_gcm_inputs(ncol, nlay, config, col0=41)
    idrv = d["idrv"]
    if case.startswith("nomcica") or case == "aer_idrv":
        icld = int(case[-1]) if case.startswith("nomcica") else 1
        plain = hip.rrtmg_lw_from_dict(d, icld=icld)
        got = hip.rrtmg_lw_from_dict(d, icld=icld, out=_nan_out(ncol, nlay, idrv), spectral=True)
    elif case == "mcica arrays":
        dd = _with_subcolumns(oracle, d, 2)
        plain = hip.rrtmg_lw_mcica_from_dict(dd, icld=2)
        got = hip.rrtmg_lw_mcica_from_dict(dd, icld=2, spectral=True, out=_spec_only(ncol, nlay))
    else:
        irng = 1 if case.endswith("mersenne") else 0
        plain = hip.rrtmg_lw_mcica_subcol_from_dict(d, 280, irng, icld=2)
        got = hip.rrtmg_lw_mcica_subcol_from_dict(d, 280, irng, icld=2, spectral=True, out=_spec_only(ncol, nlay))
    keys = BROAD + (("duflx_dt", "duflxc_dt") if idrv == 1 else ())
    for k in keys:
        assert np.array_equal(plain[k], got[k]), (case, k)
    assert plain["icld"] == got["icld"]
    _check_sums(got, case)


# ------------------------------------------------------------------------------------------------------------ 2. sum over the bands
@pytest.mark.parametrize("config", ["cloudy", "cloudy_deep", "cloudy_scatter", "cloudy_orography", "clear"])
def test_bands_add_up_to_the_broadband_fluxes(hip, config, sweeps):
    ncol, nlay = 400, 72
    d = make_gcm_inputs(ncol, nlay, config, col0=1234)
    for icld in ((0,) if config == "clear" else (1, 2)):
        got = hip.rrtmg_lw_from_dict(d, icld=icld, out=_nan_out(ncol, nlay), spectral=True)
        _check_sums(got, f"{config} icld{icld} {sweeps}")
        if icld == 0:
            for s, c in (("uflxs", "uflxcs"), ("dflxs", "dflxcs")):
                assert np.array_equal(got[s], got[c])
        assert (got["dflxs"][:, nlay, :] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------ 3. per band vs the oracle
AMD, AMW, AVOGAD, GRAV = 28.9660, 18.0160, 6.02214199e23, 9.8066


def inatm(d, i, icld):
    """Column i of the GCM inputs as the reference's inatm prepares it (src/rrtmg_lw_rad.nomcica.f90:591-919): the prepared-column
    dict of rrtmg_lw_amd.io_rrtm.read_input_rrtm."""
    nl = d["nlay"]
    g = lambda k: np.asarray(d[k][i], dtype=np.float64)
    pz, tz = g("plev"), g("tlev")
    wkl = np.zeros((7, nl))
    wkl[0], wkl[1], wkl[2], wkl[3], wkl[5], wkl[6] = g("h2ovmr"), g("co2vmr"), g("o3vmr"), g("n2ovmr"), g("ch4vmr"), g("o2vmr")
    coldry = np.empty(nl)
    for l in range(nl):
        amm = (1.0 - wkl[0, l]) * AMD + wkl[0, l] * AMW
        coldry[l] = (pz[l] - pz[l + 1]) * 1.e3 * AVOGAD / (1.e2 * GRAV * amm * (1.0 + wkl[0, l]))
    wx = np.stack([g("ccl4vmr"), g("cfc11vmr"), g("cfc12vmr"), g("cfc22vmr")])
    wbrodl = np.empty(nl)
    amttl = wvttl = 0.0
    for l in range(nl):
        summol = 0.0
        for m in range(1, 7):
            summol = summol + wkl[m, l]
        wbrodl[l] = coldry[l] * (1.0 - summol)
        wkl[:, l] = coldry[l] * wkl[:, l]
        amttl = amttl + coldry[l] + wkl[0, l]
        wvttl = wvttl + wkl[0, l]
        wx[:, l] = coldry[l] * wx[:, l] * 1.e-20
    wvsh = (AMW * wvttl) / (AMD * amttl)
    cloud = icld >= 1
    z = lambda *s: np.zeros(s)
    return dict(nlayers=nl, pavel=g("play"), tavel=g("tlay"), pz=pz, tz=tz, tbound=float(d["tsfc"][i]), semiss=g("emis"),
                coldry=coldry, wkl=wkl, wbrodl=wbrodl, wx=wx, pwvcm=wvsh * (1.e3 * pz[0]) / (1.e2 * GRAV),
                inflag=d["inflglw"] if cloud else 0, iceflag=d["iceflglw"] if cloud else 0, liqflag=d["liqflglw"] if cloud else 0,
                cldfrac=g("cldfr") if cloud else z(nl), tauc=np.asarray(d["taucld"][:, i, :]) if cloud else z(16, nl),
                ciwp=g("cicewp") if cloud else z(nl), clwp=g("cliqwp") if cloud else z(nl), rei=g("reice") if cloud else z(nl),
                rel=g("reliq") if cloud else z(nl), tauaer=np.asarray(d["tauaer"][i]), icld=icld, idrv=d["idrv"])


def _bands_of(run):
    """per band b (1-based) the column driver's result for that band alone; band 16 as its share of the bands 15-16 run"""
    res = {b: run(b, b) for b in range(1, 16)}
    both = run(15, 16)
    res[16] = {k: both[k] - res[15][k] for k in ("totuflux", "totdflux", "totuclfl", "totdclfl")}
    return res


def _compare_bands(got, i, bands, tag):
    for b in range(1, 17):
        for s, r in (("uflxs", "totuflux"), ("dflxs", "totdflux"), ("uflxcs", "totuclfl"), ("dflxcs", "totdclfl")):
            err = np.abs(got[s][i, :, b - 1] - bands[b][r]).max()
            assert err <= BAND_TOL, (tag, i, b, s, err)


@pytest.mark.parametrize("config,icld", [("cloudy", 1), ("cloudy", 2), ("cloudy_scatter", 2), ("clear", 0), ("aer_idrv", 2)])
def test_each_band_matches_the_oracle(hip, oracle, config, icld):
    ncol, nlay = 70, 40
    d = make_gcm_inputs(ncol, nlay, config, col0=555)
    got = hip.rrtmg_lw_from_dict(d, icld=icld, out=_nan_out(ncol, nlay, d["idrv"]), spectral=True)
    for i in (0, 33, 69):
        col = inatm(d, i, icld)
        bands = _bands_of(lambda a, b: oracle.column(col, a, b, iout=99))
        _compare_bands(got, i, bands, f"{config} icld{icld}")


def test_each_band_matches_the_oracle_mcica(hip, oracle):
    ncol, nlay = 50, 40
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=99)
    dd = _with_subcolumns(oracle, d, 2)
    got = hip.rrtmg_lw_mcica_from_dict(dd, icld=2, spectral=True, out=_spec_only(ncol, nlay))
    for i in (0, 17, 49):
        col = inatm(d, i, 2)
        sub = dict(cldfmc=dd["cldfmcl"][:, i, :], taucmc=dd["taucmcl"][:, i, :], ciwpmc=dd["ciwpmcl"][:, i, :],
                   clwpmc=dd["clwpmcl"][:, i, :], reicmc=dd["reicmcl"][i], relqmc=dd["relqmcl"][i])
        bands = _bands_of(lambda a, b: oracle.column_mc(col, sub, a, b, iout=99))
        _compare_bands(got, i, bands, "mcica")


def test_each_band_matches_the_reference_fortran(hip):
    from oracle.bindings import Reference
    if not Reference.available():
        pytest.skip("the reference's own Fortran build (oracle/_ref) is not present")
    ncol, nlay = 8, 40
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=7)
    got = hip.rrtmg_lw_from_dict(d, icld=2, out=_nan_out(ncol, nlay), spectral=True)
    ref = Reference()
    for i in (0, 7):
        col = inatm(d, i, 2)
        _compare_bands(got, i, _bands_of(lambda a, b: ref.column(col, a, b, iout=99)), "reference")


# ------------------------------------------------------------------------------------------------------------ 4. independence
def test_band_fluxes_do_not_depend_on_the_schedule(hip):
    ncol, nlay = 900, 60
    d = make_gcm_inputs(ncol, nlay, "cloudy_scatter", col0=3)
    runs = {}
    prev_one, prev_min = hip.set_one_sweep_max(0), hip.column_sort_min()
    prev_sort = hip.set_column_sort(True, 1 << 24)
    try:
        for name, one, sort, batch in (("three", 0, 1 << 24, None), ("one", 1 << 30, 1 << 24, None), ("sorted", 0, 0, None),
                                       ("batches", 0, 1 << 24, 256)):
            hip.set_one_sweep_max(one)
            hip.set_column_sort(True, sort)
            if batch:
                hip.set_batch(batch)
            try:
                runs[name] = hip.rrtmg_lw_from_dict(d, icld=2, out=_nan_out(ncol, nlay), spectral=True)
            finally:
                if batch:
                    hip.set_batch(0)
    finally:
        hip.set_one_sweep_max(prev_one)
        hip.set_column_sort(prev_sort, prev_min)
    for name, r in runs.items():
        for k in SPEC:
            assert np.array_equal(r[k], runs["three"][k]), (name, k)
    # one column alone against the same column inside the call
    one = {k: d[k] if not isinstance(d[k], np.ndarray) else d[k] for k in d}
    i = 517
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            one[k] = np.asfortranarray(v[:, i:i + 1, :] if k == "taucld" else v[i:i + 1])
    one["ncol"] = 1
    alone = hip.rrtmg_lw_from_dict(one, icld=2, out=_nan_out(1, nlay), spectral=True)
    for k in SPEC:
        assert np.array_equal(alone[k][0], runs["three"][k][i]), k


# ------------------------------------------------------------------------------------------------------------ 5. shapes and paths
@pytest.mark.parametrize("ncol,nlay", [(1, 72), (63, 72), (257, 72), (5000, 72), (40, 4), (65, 200)])
def test_shapes(hip, ncol, nlay):
    config = "clear" if nlay < 8 else "cloudy"
    d = make_gcm_inputs(ncol, nlay, config, col0=11)
    for icld in ((0,) if config == "clear" else (1, 2)):
        plain = hip.rrtmg_lw_from_dict(d, icld=icld)
        got = hip.rrtmg_lw_from_dict(d, icld=icld, out=_nan_out(ncol, nlay), spectral=True)
        for k in BROAD:
            assert np.array_equal(plain[k], got[k]), (ncol, nlay, icld, k)
        _check_sums(got, f"ncol={ncol} nlay={nlay} icld={icld}")


def _dev_out(torch, dev, ncol, nlay, idrv=0):
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    o = {k: z(nlay + 1, ncol) for k in ("uflx", "dflx", "uflxc", "dflxc")}
    o.update(hr=z(nlay, ncol), hrc=z(nlay, ncol))
    if idrv == 1:
        o.update(duflx_dt=z(nlay + 1, ncol), duflxc_dt=z(nlay + 1, ncol))
    o.update({k: z(16, nlay + 1, ncol) for k in SPEC})
    return o


def _host_view(o):
    """device outputs (column-fastest tensors) as the host entries' arrays"""
    r = {k: o[k].cpu().numpy().T for k in o if o[k] is not None}
    return r


def test_small_calls_replayed_as_a_graph_keep_their_spectral_buffers(hip):
    import torch
    dev = torch.device("cuda", 0)
    ncol, nlay = 700, 60
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=5, backend="torch", device=dev)
    dn = make_gcm_inputs(ncol, nlay, "cloudy", col0=5)
    ref = hip.rrtmg_lw_from_dict(dn, out=_nan_out(ncol, nlay), spectral=True)
    stream = torch.cuda.current_stream().cuda_stream
    outs = [_dev_out(torch, dev, ncol, nlay) for _ in range(2)]
    prev = hip.set_graph_max(1 << 20)
    try:
        c0, r0 = hip.graph_stats()
        for n in range(8):
            o = outs[n % 2]
            for k in SPEC:
                o[k].fill_(float("nan"))
            hip.rrtmg_lw_device(d, o, stream=stream)
            hip.check(stream)
            got = _host_view(o)
            for k in SPEC:
                assert np.array_equal(got[k], ref[k]), (n, k)
        c1, r1 = hip.graph_stats()
        assert c1 - c0 >= 2 and r1 - r0 >= 2, "the calls were not replayed from graphs"
    finally:
        hip.set_graph_max(prev)


@pytest.mark.parametrize("entry", ["nomcica", "mcica", "fused"])
def test_device_entries_on_a_caller_stream(hip, oracle, entry):
    import torch
    dev = torch.device("cuda", 0)
    ncol, nlay = 1500, 72
    config = "aer_idrv" if entry == "nomcica" else "cloudy"
    dn = make_gcm_inputs(ncol, nlay, config, col0=9)
    d = make_gcm_inputs(ncol, nlay, config, col0=9, backend="torch", device=dev)
    o = _dev_out(torch, dev, ncol, nlay, dn["idrv"])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    hip.set_batch(512)
    try:
        with torch.cuda.stream(side):
            if entry == "nomcica":
                hip.rrtmg_lw_device(d, o, stream=side.cuda_stream)
                ref = hip.rrtmg_lw_from_dict(dn, out=_nan_out(ncol, nlay, dn["idrv"]), spectral=True)
            elif entry == "mcica":
                dd = _with_subcolumns(oracle, dn, 2)
                sub = {}
                for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "taucmcl"):
                    sub[k] = torch.from_numpy(np.ascontiguousarray(dd[k].transpose(2, 1, 0))).to(dev)      # (nlay, ncol, ngpt)
                for k in ("reicmcl", "relqmcl"):
                    sub[k] = torch.from_numpy(np.ascontiguousarray(dd[k].T)).to(dev)
                hip.rrtmg_lw_mcica_device(d, sub, o, icld=2, stream=side.cuda_stream)
                ref = hip.rrtmg_lw_mcica_from_dict(dd, icld=2, spectral=True, out=_spec_only(ncol, nlay))
            else:
                hip.rrtmg_lw_mcica_subcol_device(d, o, 140, 0, icld=2, stream=side.cuda_stream)
                ref = hip.rrtmg_lw_mcica_subcol_from_dict(dn, 140, 0, icld=2, spectral=True, out=_spec_only(ncol, nlay))
        hip.check(side.cuda_stream)
    finally:
        hip.set_batch(0)
    got = _host_view(o)
    for k in BROAD + SPEC:
        assert np.array_equal(got[k], ref[k]), (entry, k)


def test_host_entries_pinned_pageable_and_three_devices(hip):
    ncol, nlay = 1100, 40
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=8)
    pageable = hip.rrtmg_lw_from_dict(d, out=_nan_out(ncol, nlay), spectral=True)
    _check_sums(pageable, "pageable")
    pinned_out = _nan_out(ncol, nlay)
    for k in SPEC:
        hip.host_register(pinned_out[k])
    try:
        pinned = hip.rrtmg_lw_from_dict(d, out=pinned_out, spectral=True)
    finally:
        for k in SPEC:
            hip.host_unregister(pinned_out[k])
    total_only = hip.rrtmg_lw_from_dict(d, out=_nan_out(ncol, nlay, clear=False), spectral=True)
    fused = hip.rrtmg_lw_mcica_subcol_from_dict(d, 7, 0, icld=2, spectral=True, out=_spec_only(ncol, nlay))
    try:
        hip.init_devices([0, 0, 0], kdata=hip.STANDIN_KDATA)
        three = hip.rrtmg_lw_from_dict(d, out=_nan_out(ncol, nlay), spectral=True)
        three_fused = hip.rrtmg_lw_mcica_subcol_from_dict(d, 7, 0, icld=2, spectral=True, out=_spec_only(ncol, nlay))
    finally:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    for k in BROAD + SPEC:
        assert np.array_equal(pinned[k], pageable[k]), k
        assert np.array_equal(three[k], pageable[k]), k
        assert np.array_equal(three_fused[k], fused[k]), k
    for k in ("uflxs", "dflxs"):
        assert np.array_equal(total_only[k], pageable[k]), k


# ------------------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors_leave_the_library_usable(hip):
    import ctypes as C
    ncol, nlay = 20, 30
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=2)
    out = _nan_out(ncol, nlay)
    base = hip.rrtmg_lw_from_dict(d, out=_nan_out(ncol, nlay), spectral=True)
    null = C.cast(None, hip._dp)
    a = [np.asfortranarray(d[k], dtype=np.float64) for k in hip._GCM_ORDER]
    c = [np.asfortranarray(d[k], dtype=np.float64) for k in hip._CLD_ORDER]
    icld = C.c_int(2)
    head = [C.c_int(ncol), C.c_int(nlay), C.byref(icld), C.c_int(0)] + [hip._p(x) for x in a]
    head += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))] + [hip._p(x) for x in c]
    head += [hip._p(out[k]) for k in BROAD] + [null, null]
    sp = [hip._p(out[k]) for k in SPEC]
    lib = hip.lib()
    for bad in ([null, sp[1], sp[2], sp[3]], [sp[0], null, sp[2], sp[3]], [sp[0], sp[1], sp[2], null], [sp[0], sp[1], null, sp[3]]):
        assert lib.rrtmg_lw_hip_run_nomcica_spectral(*head, *bad) == 2       # RRTMG_LW_HIP_EARG
        assert b"spectral" in lib.rrtmg_lw_hip_last_error()
    with pytest.raises(hip.RrtmgLwError):
        hip._check(lib.rrtmg_lw_hip_run_nomcica_spectral(*head, null, null, null, null))
    with pytest.raises(ValueError):
        hip.rrtmg_lw_from_dict(d, out=dict(_nan_out(ncol, nlay), uflxs=np.zeros((ncol, nlay + 1, 16), order="C")), spectral=True)
    again = hip.rrtmg_lw_from_dict(d, out=_nan_out(ncol, nlay), spectral=True)
    for k in BROAD + SPEC:
        assert np.array_equal(again[k], base[k]), k
