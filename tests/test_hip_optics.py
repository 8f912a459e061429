"""Gas optics and Planck sources (include/rrtmg_lw_hip.h, "Gas optics and Planck sources"): taumol's taug and fracs per g-point and
setcoef's Planck integrals per band, from the GCM, device and prepared-column entries.  Pinned against the reference's own Fortran (the
taug / fracs of tests/golden/ref_col_*.npz and ref_g256_col_*.npz), against the oracle's column driver on GCM inputs (inatm restated in
numpy), against a numpy restatement of setcoef's Planck interpolation, and against the solver itself (the surface emission the sweeps
form from these very arrays)."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

from rrtmg_lw_amd.blob import read_blob
from rrtmg_lw_amd.io_rrtm import read_input_rrtm
from rrtmg_lw_amd.synth import make_gcm_inputs, make_stress_inputs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_spectral import inatm  # noqa: E402  (inatm restated in numpy: GCM inputs -> the column driver's prepared column)

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
STATIC = read_blob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rrtmg_lw_amd", "data", "lw_static.bin"))
RTOL = 1e-12            # taug / fracs against the reference: the sums over the table rows are associated differently (observed: <= 0.15 of this bar)
FLOOR = 1e-14           # ... plus this much of the largest |value| of the layer's band
PLANCK_RTOL = 1e-13
KEYS = ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt")


def _bands(ng):
    ngc = STATIC["ngc"] if ng == 140 else np.full(16, 16)
    return np.repeat(np.arange(16), ngc)


def _err(got, ref, rtol, floor=FLOOR):
    """largest |got - ref| in units of the bar rtol |ref| + floor max_{g in band} |ref| (per layer); <= 1 passes.  got, ref: (nlay, ng)"""
    ref = np.asarray(ref, dtype=np.float64)
    band = _bands(ref.shape[1])
    bmax = np.zeros((ref.shape[0], 16))
    np.maximum.at(bmax, (slice(None), band), np.abs(ref))
    bar = rtol * np.abs(ref) + floor * bmax[:, band]
    d = np.abs(got - ref)
    assert np.isfinite(got).all()
    return float(np.max(np.where(bar > 0, d / np.where(bar > 0, bar, 1.0), np.where(d > 0, np.inf, 0.0))))


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


def _fixture_column(f):
    j = lambda n: os.path.join(G, n) if n else None
    return read_input_rrtm(j(str(f["inp"])), j(str(f["cld"])), j(str(f["aer"])))


# ------------------------------------------------------------------------------------------------------------ 1. the reference's Fortran
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(G, "ref_col_*.npz"))), ids=os.path.basename)
def test_prepared_columns_match_the_reference_fortran(hip, path):
    f = np.load(path)
    col = _fixture_column(f)
    got = hip.gas_optics_columns([col], idrv=int(col["idrv"]))
    et, ef = _err(got["taug"][0], f["taug"], RTOL), _err(got["fracs"][0], f["fracs"], RTOL)
    print(f"{os.path.basename(path)}: max rel |d taug| = {_rel(got['taug'][0], f['taug']):.2e}, fracs {_rel(got['fracs'][0], f['fracs']):.2e}"
          f" (bar use {et:.3f} / {ef:.3f})")
    assert et <= 1.0 and ef <= 1.0


@pytest.fixture()
def hip256(hip):
    hip.select_gpoints(256)
    try:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        yield hip
        hip.finalize(selected_only=True)
    finally:
        hip.select_gpoints(140)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(G, "ref_g256_col_*.npz"))), ids=os.path.basename)
def test_g256_prepared_columns_match_the_reference_fortran(hip256, path):
    f = np.load(path)            # (stored as float32)
    col = _fixture_column(f)
    got = hip256.gas_optics_columns([col], idrv=int(col["idrv"]))
    assert got["taug"].shape == (1, int(col["nlayers"]), 256)
    for k in ("taug", "fracs"):
        ref = f[k].astype(np.float64)
        assert _err(got[k][0], ref, 1e-6, 0.0) <= 1.0, k


# ------------------------------------------------------------------------------------------------------------ 2. GCM entry vs the oracle
CASES = [("clear", 72, 120, 0), ("cloudy", 72, 150, 3), ("aer_idrv", 60, 90, 5), ("aer_idrv", 137, 70, 7), ("cloudy_orography", 72, 341, 282237)]
STRESS = [("alllower", 40, 70), ("allupper", 40, 70), ("cold", 50, 70), ("hot", 50, 70), ("highgas", 50, 70)]


def _against_oracle(hip, oracle, d, cols, tag):
    got = hip.gas_optics(d, idrv=int(d["idrv"]))
    worst = [0.0, 0.0]
    for i in cols:
        ref = oracle.column(inatm(d, i, 0))
        for n, k in enumerate(("taug", "fracs")):
            e = _err(got[k][i], ref[k], RTOL)
            worst[n] = max(worst[n], e)
            assert e <= 1.0, (tag, i, k, e)
    print(f"{tag}: bar use taug {worst[0]:.3f} fracs {worst[1]:.3f}")
    return got


@pytest.mark.parametrize("config,nlay,ncol,col0", CASES, ids=[f"{c[0]}-L{c[1]}" for c in CASES])
def test_gcm_entry_matches_the_oracle(hip, oracle, config, nlay, ncol, col0):
    d = make_gcm_inputs(ncol, nlay, config, col0=col0)
    _against_oracle(hip, oracle, d, sorted({0, ncol // 2, 255 % ncol, ncol - 1}), f"{config} L{nlay}")


@pytest.mark.parametrize("kind,nlay,ncol", STRESS, ids=[s[0] for s in STRESS])
def test_stress_inputs_match_the_oracle(hip, oracle, kind, nlay, ncol):
    d = make_stress_inputs(kind, ncol, nlay, col0=17)
    got = _against_oracle(hip, oracle, d, (0, ncol // 3, ncol - 1), kind)      # (alllower: laytrop = nlay, allupper: laytrop = 0)
    assert np.isfinite(got["taug"]).all()


# ------------------------------------------------------------------------------------------------------------ 3. Planck integrals
def _interp(tab, t):
    """setcoef :173-269: tab (181, 16) at temperatures t (...) -> (..., 16)"""
    x = np.asarray(t, dtype=np.float64) - 159.0
    ind = np.clip(np.trunc(x).astype(int), 1, 180)
    f = (x - ind)[..., None]
    return tab[ind - 1] + f * (tab[ind] - tab[ind - 1])


def _planck_ref(d):
    tp, td = STATIC["totplnk"].reshape(181, 16), STATIC["totplnkderiv"].reshape(181, 16)
    emis = np.asarray(d["emis"])
    return dict(planklay=_interp(tp, d["tlay"]), planklev=_interp(tp, d["tlev"]), plankbnd=emis * _interp(tp, d["tsfc"]),
                dplankbnd_dt=emis * _interp(td, d["tsfc"]))


def _per_band_emis(d, seed):
    d["emis"] = np.asfortranarray(np.random.default_rng(seed).uniform(0.7, 1.0, np.asarray(d["emis"]).shape))
    return d


@pytest.mark.parametrize("config,idrv", [("cloudy", 0), ("aer_idrv", 1)])
def test_planck_integrals_match_setcoef(hip, config, idrv):
    ncol, nlay = 300, 72
    d = _per_band_emis(make_gcm_inputs(ncol, nlay, config, col0=12), 4)
    d["tlay"] = np.asfortranarray(np.asarray(d["tlay"]) + np.linspace(-80, 80, ncol)[:, None])       # beyond both ends of the table
    d["tlev"] = np.asfortranarray(np.asarray(d["tlev"]) + np.linspace(-80, 80, ncol)[:, None])
    got = hip.gas_optics(d, idrv=idrv)
    ref = _planck_ref(d)
    for k in ("planklay", "planklev", "plankbnd") + (("dplankbnd_dt",) if idrv else ()):
        assert got[k].shape == ref[k].shape, k
        # (rounding of the interpolation's terms: relative to the band's largest value where the extrapolation below 160 K cancels)
        atol = PLANCK_RTOL * np.abs(ref[k]).max(axis=tuple(range(ref[k].ndim - 1)), keepdims=True)
        assert (np.abs(got[k] - ref[k]) <= PLANCK_RTOL * np.abs(ref[k]) + atol).all(), (k, np.abs(got[k] - ref[k]).max())
    assert "dplankbnd_dt" in got if idrv else "dplankbnd_dt" not in got
    # band 16 is the broadband call's (istart = 1): the totplnk row, not totplk16
    tp16 = STATIC["totplk16"].reshape(181)
    assert not np.allclose(got["plankbnd"][:, 15], np.asarray(d["emis"])[:, 15] * _interp(tp16[:, None], d["tsfc"])[:, 0], rtol=1e-6, atol=0)


def test_null_planck_outputs_are_left_alone(hip):
    ncol, nlay = 200, 50
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=2)
    full = hip.gas_optics(d, idrv=1)
    shapes = {k: full[k].shape for k in KEYS}
    nan = lambda k: np.full(shapes[k], np.nan, order="F")
    # idrv = 0: dplankbnd_dt may be given and stays as it was
    out = {k: nan(k) for k in KEYS}
    got = hip.gas_optics(d, idrv=0, out=out)
    assert np.isnan(got["dplankbnd_dt"]).all()
    for k in KEYS[:5]:
        assert np.array_equal(got[k], full[k]), k
    # no Planck outputs at all: taug and fracs as before
    out = dict(taug=nan("taug"), fracs=nan("fracs"), planklay=None, planklev=None, plankbnd=None)
    got = hip.gas_optics(d, idrv=0, out=out)
    for k in ("taug", "fracs"):
        assert np.array_equal(got[k], full[k]), k
    # some of them
    out = dict(taug=nan("taug"), fracs=nan("fracs"), planklay=None, planklev=nan("planklev"), plankbnd=None)
    got = hip.gas_optics(d, idrv=0, out=out)
    for k in ("taug", "fracs", "planklev"):
        assert np.array_equal(got[k], full[k]), k


# ------------------------------------------------------------------------------------------------------------ 4. the solver's arrays
@pytest.mark.parametrize("config", ["clear", "cloudy_orography"])
def test_surface_emission_of_the_solver(hip, config):
    """With emis = 1 the solver's upward flux at the surface is pi 1e4 sum_b delwave_b plankbnd_b sum_{g in b} fracs(1, g)
    (src/rrtmg_lw_rtrn.f90:476-489,549-562; tests/test_golden_planck.py).  The sweeps carry the mixture weight of the Planck fractions
    in 28 bits (kernels.hip: Rows::fw): ~1e-9 of a fraction."""
    ncol, nlay = 300, 72
    d = make_gcm_inputs(ncol, nlay, config, col0=44)
    d["emis"] = np.ones((ncol, 16), order="F")
    flux = hip.rrtmg_lw_from_dict(d, icld=0, idrv=0)["uflx"][:, 0]
    o = hip.gas_optics(d)
    band = _bands(o["fracs"].shape[2])
    fsum = np.zeros((ncol, 16))
    np.add.at(fsum, (slice(None), band), o["fracs"][:, 0, :])
    want = np.pi * 1e4 * (STATIC["delwave"][None, :] * o["plankbnd"] * fsum).sum(axis=1)
    np.testing.assert_allclose(flux, want, rtol=1e-8, atol=0)


# ------------------------------------------------------------------------------------------------------------ 5. independence
def _cols(d, sl):
    o = dict(d)
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            o[k] = np.asfortranarray(v[:, sl] if k == "taucld" else v[sl])
    o["ncol"] = len(range(*sl.indices(d["ncol"])))
    return o


def _same(a, b, tag, keys=KEYS):
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k]), (tag, k)


def test_batches_and_single_columns_agree(hip):
    ncol, nlay = 150, 60
    d = make_gcm_inputs(ncol, nlay, "cloudy_orography", col0=9)
    hip.set_batch(64)
    try:
        batched = hip.gas_optics(d, idrv=0)
    finally:
        hip.set_batch(0)
    for i in range(ncol):
        one = hip.gas_optics(_cols(d, slice(i, i + 1)))
        for k in KEYS[:5]:
            assert np.array_equal(one[k][0], batched[k][i]), (i, k)


def test_ragged_last_window(hip):
    nlay = 72
    d = make_gcm_inputs(600, nlay, "cloudy_orography", col0=282237)
    whole = hip.gas_optics(d)
    part = hip.gas_optics(_cols(d, slice(0, 300)))           # windows of 256 + 44 columns
    for k in KEYS[:5]:
        assert np.array_equal(part[k], whole[k][:300]), k
    tail = hip.gas_optics(_cols(d, slice(557, 600)))         # one window of 43
    for k in KEYS[:5]:
        assert np.array_equal(tail[k], whole[k][557:]), k


def test_device_entry_on_a_caller_stream(hip):
    import torch
    dev = torch.device("cuda", 0)
    ncol, nlay = 1500, 72
    dn = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=9)
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=9, backend="torch", device=dev)
    ng = hip.gpoints()
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    o = dict(taug=z(ng, nlay, ncol), fracs=z(ng, nlay, ncol), planklay=z(16, nlay, ncol), planklev=z(16, nlay + 1, ncol),
             plankbnd=z(16, ncol), dplankbnd_dt=z(16, ncol))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    hip.set_batch(512)
    try:
        with torch.cuda.stream(side):
            hip.gas_optics_device(d, o, stream=side.cuda_stream)
        hip.check(side.cuda_stream)
    finally:
        hip.set_batch(0)
    ref = hip.gas_optics(dn, idrv=1)
    for k in KEYS:
        assert np.array_equal(o[k].cpu().numpy().T, ref[k]), k


def test_three_devices_and_one_agree(hip):
    ncol, nlay = 1100, 40
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=8)
    one = hip.gas_optics(d, idrv=1)
    try:
        hip.init_devices([0, 0, 0], kdata=hip.STANDIN_KDATA)
        three = hip.gas_optics(d, idrv=1)
    finally:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    _same(three, one, "three devices")


# ------------------------------------------------------------------------------------------------------------ 6. errors and memory
def test_argument_errors_leave_the_library_usable(hip):
    ncol, nlay = 20, 30
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=2)
    base = hip.gas_optics(d, idrv=1)
    lib = hip.lib()
    null = C.cast(None, hip._dp)
    ins = [hip._p(np.asfortranarray(d[k], dtype=np.float64)) for k in hip._GCM_ORDER]
    keep = {k: np.empty_like(base[k], order="F") for k in KEYS}
    outs = [hip._p(keep[k]) for k in KEYS]
    call = lambda n, L, idrv, o: lib.rrtmg_lw_hip_gas_optics(C.c_int(n), C.c_int(L), C.c_int(idrv), *ins, *o)
    assert call(ncol, nlay, 1, outs) == 0
    for bad in ([null] + outs[1:], outs[:1] + [null] + outs[2:]):
        assert call(ncol, nlay, 0, bad) == 2                                # RRTMG_LW_HIP_EARG
        assert b"taug and fracs" in lib.rrtmg_lw_hip_last_error()
    assert call(ncol, nlay, 1, outs[:5] + [null]) == 2
    assert b"dplankbnd_dt" in lib.rrtmg_lw_hip_last_error()
    assert call(0, nlay, 0, outs) == 2 and call(ncol, 0, 0, outs) == 2 and call(ncol, 604, 0, outs) == 2
    assert lib.rrtmg_lw_hip_gas_optics(C.c_int(ncol), C.c_int(nlay), C.c_int(0), *ins[:3], null, *ins[4:], *outs) == 2
    cn = [null] * 11
    assert lib.rrtmg_lw_hip_gas_optics_columns(C.c_int(1), C.c_int(nlay), C.c_int(0), *cn, null, null, null, null, null, null) == 2
    assert lib.rrtmg_lw_hip_gas_optics_device(C.c_int(ncol), C.c_int(nlay), C.c_int(0), *ins, null, null, null, null, null, null,
                                              C.c_void_p(0)) == 2
    with pytest.raises(ValueError):
        hip.gas_optics(d, out=dict(taug=np.zeros(base["taug"].shape, order="C")))
    with pytest.raises(ValueError):
        hip.gas_optics(d, out=dict(taug=None))
    _same(hip.gas_optics(d, idrv=1), base, "after the errors")


def test_optics_calls_do_not_allocate_the_solver_workspace(hip):
    import torch
    dev = torch.device("cuda", 0)
    ncol, nlay = 4096, 72
    d = make_gcm_inputs(ncol, nlay, "clear", col0=3, backend="torch", device=dev)
    ng = hip.gpoints()
    e = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    try:
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        hip.gas_optics_device(d, dict(taug=e(ng, nlay, ncol), fracs=e(ng, nlay, ncol), planklay=e(16, nlay, ncol),
                                      planklev=e(16, nlay + 1, ncol), plankbnd=e(16, ncol)))
        hip.check()
        optics = hip.workspace_bytes()
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        out = {k: e(nlay + 1, ncol) for k in ("uflx", "dflx", "uflxc", "dflxc")}
        out.update(hr=e(nlay, ncol), hrc=e(nlay, ncol))
        hip.rrtmg_lw_device(d, out, icld=0, idrv=0)
        hip.check()
        clear = hip.workspace_bytes()
    finally:
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    print(f"workspace after an optics call {optics} B, after a clear-sky rrtmg_lw call {clear} B ({ncol} x {nlay})")
    assert 0 < optics < clear / 10
