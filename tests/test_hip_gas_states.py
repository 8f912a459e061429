"""The HIP path on the designed gas states (tests/gas_states.py; ledger and CPU half in tests/test_gas_state_coverage.py): k_optics and
the solver against the oracle for EVERY column of the set, against the committed reference-made fixture, the prepared-column entries
with CO and the halocarbons varied, independence of the column order / staging window / batch split, and the 256-g-point library.
Every comparison prints the use of its bar (worst error over bar); a failure names band, layer, g-point and the cell's decisions."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gas_states as gs  # noqa: E402
from test_gas_state_coverage import FIXTURE, NLAY, SEED  # noqa: E402
from test_hip_optics import FLOOR, KEYS, PLANCK_RTOL, RTOL, _bands, _err, _planck_ref  # noqa: E402
from test_hip_spectral import BAND_TOL, BROAD, SPEC, _nan_out, inatm  # noqa: E402

pytestmark = pytest.mark.gpu

BAND_STRIDE = 6          # per-band fluxes: the oracle runs one band at a time (17 runs a column), so every 6th column of the shuffled set


@pytest.fixture(scope="module")
def states():
    return gs.make_gas_states(NLAY, SEED, "shuffled")


@pytest.fixture(scope="module")
def dec(states):
    return gs.decisions(states)


_CACHE = {}


def _oracle_columns(oracle, d, tag="140"):
    """oracle.column of every converted column, computed once and left unchanged"""
    if tag not in _CACHE:
        _CACHE[tag] = [oracle.column(inatm(d, i, 0)) for i in range(d["ncol"])]
    return _CACHE[tag]


def _oracle_gcm(oracle, d, icld, idrv):
    key = ("gcm", icld, idrv)
    if key not in _CACHE:
        _CACHE[key] = oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, idrv, d)
    return _CACHE[key]


def _oracle_bands(oracle, d, icld):
    """{column: {band: fluxes of that band alone}} for every BAND_STRIDE-th column (band 16 in the broadband call's convention)"""
    key = ("bands", icld)
    if key not in _CACHE:
        res = {}
        for i in range(0, d["ncol"], BAND_STRIDE):
            col = inatm(d, i, icld)
            r = {b: oracle.column(col, b, b, iout=99) for b in range(1, 16)}
            both = oracle.column(col, 15, 16, iout=99)
            r[16] = {k: both[k] - r[15][k] for k in ("totuflux", "totdflux", "totuclfl", "totdclfl")}
            res[i] = r
        _CACHE[key] = res
    return _CACHE[key]


def _name_cell(got, ref, k, i, d, dec):
    """band, layer, g-point of the worst cell of column i and what setcoef / taumol decided there"""
    lay = int(np.argmax([_err(got[l:l + 1], ref[l:l + 1], RTOL) for l in range(ref.shape[0])]))
    one = []
    for g in range(ref.shape[1]):
        x = np.array(ref[lay:lay + 1], dtype=np.float64)
        x[0, g] = got[lay, g]
        one.append(_err(x, ref[lay:lay + 1], RTOL))
    g = int(np.argmax(one))
    band = int(_bands(ref.shape[1])[g]) + 1
    return (f"{k}: column {i} ({d['labels'][i]}), band {band}, layer {lay + 1}, g-point {g + 1}: got {got[lay, g]!r}, oracle {ref[lay, g]!r}, "
            f"{max(one):.3g} x bar; decisions {gs.decision_row(dec, i, lay)}")


def _compare_optics(got, refs, d, dec, tag, cols=None):
    worst = {"taug": 0.0, "fracs": 0.0}
    for n, i in enumerate(range(d["ncol"]) if cols is None else cols):
        for k in worst:
            e = _err(got[k][n], refs[i][k], RTOL)
            assert e <= 1.0, _name_cell(got[k][n], refs[i][k], k, i, d, dec)
            worst[k] = max(worst[k], e)
    print(f"{tag}: bar use taug {worst['taug']:.3f} fracs {worst['fracs']:.3f}")


def _compare_planck(got, d, idrv):
    ref = _planck_ref(d)
    use = 0.0
    for k in ("planklay", "planklev", "plankbnd") + (("dplankbnd_dt",) if idrv else ()):
        atol = PLANCK_RTOL * np.abs(ref[k]).max(axis=tuple(range(ref[k].ndim - 1)), keepdims=True)      # (tests/test_hip_optics.py)
        r = np.abs(got[k] - ref[k]) / (PLANCK_RTOL * np.abs(ref[k]) + atol)
        assert (r <= 1.0).all(), (k, float(r.max()))
        use = max(use, float(r.max()))
    print(f"planck integrals: bar use {use:.3f}")


def _compare_fluxes(got, ref, plev, idrv, tag, labels):
    """the bars of tests/test_fuzz.py::test_random_terrain_calls: fluxes within max(5e-5, 2.5e-7 scale), heating rates in the thin-layer form"""
    keys = ("uflx", "dflx", "uflxc", "dflxc") + (("duflx_dt", "duflxc_dt") if idrv else ())
    scale = max(np.abs(ref[k]).max() for k in ("uflx", "dflx"))
    bar = max(5e-5, 2.5e-7 * scale)
    use_f = 0.0
    for k in keys:
        err = np.abs(got[k] - ref[k])
        i = int(np.argmax(err.max(axis=1)))
        assert err.max() <= bar, (tag, k, float(err.max()), bar, i, labels[i])
        use_f = max(use_f, float(err.max()) / bar)
    dp = plev[:, :-1] - plev[:, 1:]
    use_h = 0.0
    for k in ("hr", "hrc"):
        err = np.abs(got[k] - ref[k])
        hbar = np.maximum(5e-5, 2.5e-5 * 8.4391 / dp) + 1e-6 * np.abs(ref[k])
        i = int(np.argmax((err / hbar).max(axis=1)))
        assert (err <= hbar).all(), (tag, k, float((err / hbar).max()), i, labels[i])
        assert err[dp >= 0.25].max() <= 1e-3, (tag, k)
        use_h = max(use_h, float((err / hbar).max()))
    print(f"{tag}: bar use fluxes {use_f:.3f} (bar {bar:.2e} W m-2, scale {scale:.0f}) heating rates {use_h:.3f}")


# ------------------------------------------------------------------------------------------------------------ 1. k_optics vs the oracle
def test_optics_match_the_oracle_in_every_column(hip, oracle, states, dec):
    t0 = time.time()
    got = hip.gas_optics(states, idrv=1)
    t1 = time.time()
    _compare_optics(got, _oracle_columns(oracle, states), states, dec, f"gas optics, {states['ncol']} columns")
    _compare_planck(got, states, 1)
    print(f"(library call {t1 - t0:.2f} s)")


# ------------------------------------------------------------------------------------------------------------ 2. solver vs the oracle
@pytest.mark.parametrize("icld,idrv", [(0, 0), (0, 1), (2, 0), (2, 1)])
def test_solver_matches_the_oracle(hip, oracle, states, sweeps, icld, idrv):
    d = gs.with_clouds(states) if icld else states
    ncol, nlay = d["ncol"], d["nlay"]
    got = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv, out=_nan_out(ncol, nlay, idrv), spectral=True)
    ref = _oracle_gcm(oracle, d, icld, idrv)
    assert got["icld"] == ref["icld"]
    _compare_fluxes(got, ref, np.asarray(d["plev"]), idrv, f"solver icld{icld} idrv{idrv} ({sweeps})", d["labels"])
    worst = 0.0
    for i, bands in _oracle_bands(oracle, d, icld).items():
        for b in range(1, 17):
            for s, r in (("uflxs", "totuflux"), ("dflxs", "totdflux"), ("uflxcs", "totuclfl"), ("dflxcs", "totdclfl")):
                err = np.abs(got[s][i, :, b - 1] - bands[b][r]).max()
                assert err <= BAND_TOL, (icld, i, d["labels"][i], b, s, err)
                worst = max(worst, err)
    print(f"per band (every {BAND_STRIDE}th column): bar use {worst / BAND_TOL:.3f}")


# ------------------------------------------------------------------------------------------------------------ 3. the reference's numbers
def test_optics_and_solver_match_the_reference_fixture(hip, states, dec):
    f = np.load(FIXTURE)
    cols = f["cols"]
    assert [states["labels"][i] for i in cols] == [str(s) for s in f["labels"]], "the design changed: tools/gen_ref_fixtures.py --gasstate"
    sub = gs.take(states, cols)
    got = hip.gas_optics(sub, idrv=1)
    use = 0.0
    for n, i in enumerate(cols):
        lays = f["lays"][n]
        for k in ("taug", "fracs"):
            e = _err(got[k][n][lays], f[k][n], RTOL)
            assert e <= 1.0, (k, states["labels"][i], lays, e, gs.decision_row(dec, int(i), int(lays[0])))
            use = max(use, e)
    print(f"reference fixture, {len(cols)} columns x 2 layers: bar use taug / fracs {use:.3f}")
    out = hip.rrtmg_lw_from_dict(sub, icld=0, idrv=1)
    _compare_fluxes(out, {k: f[k] for k in f.files}, np.asarray(sub["plev"]), 1, "reference fixture", sub["labels"])


# ------------------------------------------------------------------------------------------------------------ 4. prepared columns
def test_prepared_columns_with_co_and_halocarbons(hip, oracle, states, dec):
    idx, cols = gs.prepared_companion(states, inatm)
    refs = {int(i): oracle.column(c) for i, c in zip(idx, cols)}
    plain = _oracle_columns(oracle, states)
    g13 = _bands(140) == 12
    moved = [np.abs(refs[int(i)]["taug"][0, g13] / plain[int(i)]["taug"][0, g13] - 1.0).max() for i in idx if dec["lower"][i, 0]]
    assert max(moved) > 1e-3, "CO does not show in band 13: the companion tests nothing"
    got = hip.gas_optics_columns(cols, idrv=0)
    _compare_optics(got, refs, states, dec, f"prepared columns, {len(cols)} columns", cols=[int(i) for i in idx])
    run = hip.run_columns(cols, icld=0, idrv=0)
    ref = {k: np.stack([refs[int(i)][k] for i in idx]) for k in ("totuflux", "totdflux", "totuclfl", "totdclfl", "htr", "htrc")}
    names = dict(uflx="totuflux", dflx="totdflux", uflxc="totuclfl", dflxc="totdclfl")
    g = {k: run[v] for k, v in names.items()}
    r = {k: ref[v] for k, v in names.items()}
    for a, b in (("hr", "htr"), ("hrc", "htrc")):
        g[a], r[a] = run[b][:, :-1], ref[b][:, :-1]
    _compare_fluxes(g, r, np.asarray(states["plev"])[idx], 0, "prepared columns", [states["labels"][int(i)] for i in idx])


# ------------------------------------------------------------------------------------------------------------ 5. order independence
def _all_outputs(hip, d, icld=0):
    o = hip.gas_optics(d, idrv=1)
    s = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=1, out=_nan_out(d["ncol"], d["nlay"], 1), spectral=True)
    res = {k: o[k] for k in KEYS}
    res.update({k: s[k] for k in BROAD + SPEC + ("duflx_dt", "duflxc_dt")})
    return res


def _same(a, b, tag, sel_a=slice(None), sel_b=slice(None)):
    for k in a:
        assert np.array_equal(a[k][sel_a], b[k][sel_b]), (tag, k)


@pytest.fixture(scope="module")
def baseline(hip, states):
    return _all_outputs(hip, states)


def test_grouped_and_shuffled_orders_agree_bit_for_bit(hip, states, baseline):
    grouped = gs.make_gas_states(NLAY, SEED, "grouped")
    g = _all_outputs(hip, grouped)
    _same(baseline, g, "grouped vs shuffled", sel_b=states["perm"])


def test_narrow_and_wide_staging_windows_agree_bit_for_bit(hip, states, baseline):
    outs = {}
    prev = hip.set_wide_window(1)
    try:
        for on in (1, 0):
            hip.set_wide_window(on)
            outs[on] = _all_outputs(hip, states)
    finally:
        hip.set_wide_window(prev)
    _same(outs[1], outs[0], "wide vs narrow")
    _same(outs[1 if prev else 0], baseline, "default window")


def test_window_splits_agree_bit_for_bit(hip, states, baseline):
    hip.set_batch(64)
    try:
        small = _all_outputs(hip, states)
    finally:
        hip.set_batch(0)
    _same(small, baseline, "batches of 64")
    n = gs.RAGGED_END
    assert "s=clamp" in states["labels"][n - 1] and n % 256
    try:
        part = _all_outputs(hip, gs.take(states, slice(0, n)))
    finally:
        hip.set_batch(0)
    _same(part, baseline, f"first {n} columns alone", sel_b=slice(0, n))


# ------------------------------------------------------------------------------------------------------------ 6. 256 g-points
@pytest.fixture()
def hip256(hip):
    hip.select_gpoints(256)
    try:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        yield hip
        hip.finalize(selected_only=True)
    finally:
        hip.select_gpoints(140)


def test_g256_optics_and_fluxes_match_the_oracle(hip256, states, dec):
    from oracle.bindings import Oracle
    o256 = Oracle(gpoints=256)
    assert hip256.gpoints() == 256
    got = hip256.gas_optics(states, idrv=1)
    assert got["taug"].shape == (states["ncol"], NLAY, 256)
    _compare_optics(got, _oracle_columns(o256, states, "256"), states, dec, f"256 g-points, gas optics, {states['ncol']} columns")
    d = gs.with_clouds(states)
    for dd, icld in ((states, 0), (d, 2)):
        out = hip256.rrtmg_lw_from_dict(dd, icld=icld, idrv=1)
        ref = o256.rrtmg_lw(dd["ncol"], NLAY, icld, 1, dd)
        # tests/test_g256.py: fluxes within 5e-5 W m-2
        dflux = max(np.abs(out[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc", "duflx_dt", "duflxc_dt"))
        print(f"256 g-points icld{icld}: max |dflux| = {dflux:.3e} W m-2 (bar use {dflux / 5e-5:.3f})")
        assert dflux <= 5e-5
        # heating rates: the thin-layer form (the set has layers of 3 hPa, where 5e-5 K/d is less than the flux bar allows)
        _compare_fluxes(out, ref, np.asarray(dd["plev"]), 1, f"256 g-points icld{icld}", dd["labels"])
