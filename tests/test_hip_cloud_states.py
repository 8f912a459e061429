"""The HIP path on the designed cloud states (tests/cloud_states.py; ledgers and CPU half in tests/test_cloud_state_coverage.py):
k_cloudscan / k_cloudlay and k_cloudmc (array path and mask path) against the oracle for EVERY column of families A and B - broadband
and, for the table walk, per band -, against the committed reference-made fixture, with the unread out-of-bounds sizes of family C, at
and beyond every bound of cldprop's five stops (family D), and through the 256-g-point library.  Every comparison prints the use of its
bar (worst error over bar); a failure names family, table, interval, band and the column's decisions."""
import os
import sys

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_states as cs  # noqa: E402
from test_cloud_state_coverage import FIXTURE, FIXTURE_KEYS, FLUX_KEYS, _all_calls, band_runs, fixture_reference, subcolumns  # noqa: E402
from test_hip_launch_matrix import _to_device  # noqa: E402
from test_hip_parity import TIGHT_FLUX, TIGHT_HR  # noqa: E402
from test_hip_spectral import BAND_TOL, BROAD, _dev_out, _host_view, _nan_out  # noqa: E402

pytestmark = pytest.mark.gpu

SPEC_OF = (("uflxs", "totuflux"), ("dflxs", "totdflux"), ("uflxcs", "totuclfl"), ("dflxcs", "totdclfl"))
_CACHE = {}


def _cached(key, make):
    """references are computed once per module and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def calls():
    return _all_calls(cs.family_a(), cs.family_b())


@pytest.fixture(scope="module")
def decs(calls):
    return {k: cs.decisions(d) for k, d in calls.items()}


def _oracle_gcm(oracle, key, d, icld, idrv, tag="140"):
    return _cached(("gcm", tag, key, icld, idrv), lambda: oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, idrv, d))


def _oracle_bands(oracle, key, d, icld):
    """{spectral output: (ncol, nlay + 1, 16)} from the oracle's one-band runs of every column"""
    def make():
        out = {s: np.empty((d["ncol"], d["nlay"] + 1, 16)) for s, _ in SPEC_OF}
        for i in range(d["ncol"]):
            r = band_runs(oracle, d, i, icld)
            for s, k in SPEC_OF:
                for b in range(1, 17):
                    out[s][i, :, b - 1] = r[b][k]
        return out
    return _cached(("bands", key, icld), make)


def _name(d, dec, i, band=None):
    m = d["meta"][i]
    where = ""
    if m.get("table"):
        ikey = "index_i" if cs.TABLES[m["table"]]["phase"] == "ice" else "index_l"
        where = f", table {m['table']}, interval {int(dec[ikey][i, m['lay']])}"
    return (f"family {d['family']}, flags {d['inflglw']} / {d['iceflglw']} / {d['liqflglw']}, column {i}: {d['labels'][i]}{where}"
            + (f", band {band}" if band else "") + f"; decisions {cs.decision_rows(dec, i)}")


def _compare_broadband(got, ref, idrv, d, dec, tag):
    """TIGHT_FLUX on the fluxes and on d(flux)/dT, TIGHT_HR on the heating rates; returns the use of the bars"""
    use = 0.0
    for keys, bar in ((("uflx", "dflx", "uflxc", "dflxc") + (("duflx_dt", "duflxc_dt") if idrv else ()), TIGHT_FLUX), (("hr", "hrc"), TIGHT_HR)):
        for k in keys:
            assert np.isfinite(got[k]).all(), (tag, k)
            err = np.abs(got[k] - ref[k])
            if err.max() > bar:
                i, l = np.unravel_index(int(np.argmax(err)), err.shape)
                raise AssertionError(f"{tag}: {k} off by {err.max():.3e} (bar {bar:g}) at index {l} of {_name(d, dec, int(i))}")
            use = max(use, float(err.max()) / bar)
    assert got["icld"] == ref["icld"]
    return use


def _compare_bands(got, bands, d, dec, tag):
    use = 0.0
    for s, _ in SPEC_OF:
        err = np.abs(got[s] - bands[s])
        if err.max() > BAND_TOL:
            i, lev, b = np.unravel_index(int(np.argmax(err)), err.shape)
            raise AssertionError((tag, s, float(err.max()), BAND_TOL, f"level {lev}", _name(d, dec, int(i), int(b) + 1)))
        use = max(use, float(err.max()) / BAND_TOL)
    return use


# ------------------------------------------------------------------------------------------------------------ 1. families A and B
@pytest.mark.parametrize("idrv", [0, 1])
@pytest.mark.parametrize("icld", [1, 2])
@pytest.mark.parametrize("family", ["A", "B"])
def test_families_match_the_oracle(hip, oracle, calls, decs, sweeps, family, icld, idrv):
    use, use_b = 0.0, 0.0
    for key, d in calls.items():
        if key[0] != family:
            continue
        got = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv, out=_nan_out(d["ncol"], d["nlay"], idrv), spectral=True)
        tag = f"{key} icld{icld} idrv{idrv} ({sweeps})"
        use = max(use, _compare_broadband(got, _oracle_gcm(oracle, key, d, icld, idrv), idrv, d, decs[key], tag))
        if family == "A":        # every column of the walk, under the flag pair that reads its table, band by band
            use_b = max(use_b, _compare_bands(got, _oracle_bands(oracle, key, d, icld), d, decs[key], tag))
    print(f"family {family} icld{icld} idrv{idrv} ({sweeps}): bar use broadband {use:.3f}" + (f", per band {use_b:.3f}" if family == "A" else ""))


def test_families_match_the_reference_fixture(hip, calls, decs, sweeps):
    f = np.load(FIXTURE)
    use = 0.0
    for key, (cols, ref) in fixture_reference(f, calls).items():
        d = calls[key]
        got = hip.rrtmg_lw_from_dict(d, icld=2, idrv=0)
        for k in FIXTURE_KEYS:
            bar = TIGHT_HR if k == "hr" else TIGHT_FLUX
            err = np.abs(got[k][cols] - ref[k])
            assert err.max() <= bar, (key, k, float(err.max()), _name(d, decs[key], int(cols[int(np.argmax(err.max(axis=1)))])))
            use = max(use, float(err.max()) / bar)
    print(f"reference fixture, {len(f['labels'])} columns ({sweeps}): bar use {use:.3f}")


# ------------------------------------------------------------------------------------------------------------ 2. McICA
@pytest.mark.parametrize("icld", [1, 2, 3])
def test_mcica_array_and_fused_entries(hip, oracle, calls, decs, sweeps, icld):
    """cldprmc has no band count to carry, but reads the same tables at the same positions, per g-point (k_cloudmc<arrays>); the fused
    generator + solver entry draws the same kissvec sub-columns itself (k_cloudmc<mask>) and must give the array path's bits"""
    use = 0.0
    for key, d in calls.items():
        if d["inflglw"] == 1:          # not available with McICA (src/rrtmg_lw_cldprmc.f90:190)
            continue
        dd = _cached(("sub", key, icld), lambda: subcolumns(oracle, d, icld))
        ref = _cached(("mcica", key, icld), lambda: oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, 1, dd, mcica=True))
        got = hip.rrtmg_lw_mcica_from_dict(dd, icld=icld, idrv=1)
        use = max(use, _compare_broadband(got, ref, 1, d, decs[key], f"mcica arrays {key} icld{icld} ({sweeps})"))
        fused = hip.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, icld=icld, idrv=1)
        for k in BROAD + ("duflx_dt", "duflxc_dt"):
            assert np.array_equal(got[k], fused[k]), ("mask path vs array path", key, icld, k)
    print(f"mcica icld{icld} ({sweeps}): bar use {use:.3f}")


# ------------------------------------------------------------------------------------------------------------ 3. family C
def _device_call(hip, d, icld, idrv):
    import torch
    dev = torch.device("cuda", 0)
    dd = {k: _to_device(torch, dev, v) for k, v in d.items() if k != "perm"}
    o = _dev_out(torch, dev, d["ncol"], d["nlay"], idrv)
    stream = torch.cuda.current_stream().cuda_stream
    hip.rrtmg_lw_device(dd, o, icld=icld, idrv=idrv, stream=stream)
    hip.check(stream)
    return _host_view(o)


@pytest.mark.parametrize("flags", cs.C_FLAGS, ids=lambda f: "flags %d%d%d" % f)
def test_unread_sizes_change_nothing(hip, flags):
    clean, junk = _cached("C", cs.family_c)[flags]
    keys = BROAD + ("duflx_dt", "duflxc_dt")
    for icld in (1, 2):
        hip.set_batch(256)
        try:
            a, b = (hip.rrtmg_lw_from_dict(d, icld=icld, idrv=1) for d in (clean, junk))
        finally:
            hip.set_batch(0)
        da, db = (_device_call(hip, d, icld, 1) for d in (clean, junk))
        for k in keys:
            assert np.array_equal(a[k], b[k]), ("host entry", flags, icld, k)
            assert np.array_equal(da[k], db[k]), ("device entry", flags, icld, k)
            assert np.array_equal(a[k], da[k]), ("host vs device entry", flags, icld, k)
        assert np.abs(a["dflx"] - a["dflxc"]).max() > 1.0
    if flags[0] != 1:
        a, b = (hip.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, icld=2, idrv=1) for d in (clean, junk))
        for k in keys:
            assert np.array_equal(a[k], b[k]), ("fused entry", flags, k)


# ------------------------------------------------------------------------------------------------------------ 4. family D
@pytest.fixture(scope="module")
def before(hip, calls):
    """a clear call and a family-A call, made before any stop is raised"""
    clear = make_gcm_inputs(70, 40, "clear")
    walk = calls[("A", 2, 0)]
    return clear, walk, hip.rrtmg_lw_from_dict(clear, icld=0, idrv=0), hip.rrtmg_lw_from_dict(walk, icld=2, idrv=0)


def _still_the_same(hip, before, tag):
    clear, walk, rc, rw = before
    a, b = hip.rrtmg_lw_from_dict(clear, icld=0, idrv=0), hip.rrtmg_lw_from_dict(walk, icld=2, idrv=0)
    for k in BROAD:
        assert np.array_equal(a[k], rc[k]) and np.array_equal(b[k], rw[k]), (tag, k)


def _entries(hip, oracle):
    return (("non-McICA icld 1", lambda d: hip.rrtmg_lw_from_dict(d, icld=1, idrv=0)),
            ("non-McICA icld 2", lambda d: hip.rrtmg_lw_from_dict(d, icld=2, idrv=0)),
            ("McICA arrays", lambda d: hip.rrtmg_lw_mcica_from_dict(subcolumns(oracle, d, 2), icld=2, idrv=0)),
            ("McICA fused", lambda d: hip.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, icld=2, idrv=0)))


@pytest.mark.parametrize("case", cs.stop_cases(), ids=lambda c: c[0] + " iceflag %d" % c[1][0])
def test_stops_at_the_bounds(hip, oracle, before, case):
    """the bound passes, the next double beyond it raises the reference's text - and the ice text where the liquid size of the same layer
    is out as well (the reference checks ice first: src/rrtmg_lw_cldprop.f90:212-273, src/rrtmg_lw_cldprmc.f90:204-254)"""
    name, (iceflag, liqflag), phase, key, bound, beyond, msg = case
    d = cs.stop_call(iceflag, liqflag)
    col = cs.first_cloudy_column(d)
    ok, bad = cs.with_size(d, key, col, bound), cs.with_size(d, key, col, beyond)
    for entry, run in _entries(hip, oracle):
        got = run(ok)
        assert np.isfinite(got["uflx"]).all(), (entry, name)
        with pytest.raises(hip.RrtmgLwError, match=msg):
            run(bad)
        _still_the_same(hip, before, (entry, name))
        if phase == "ice":
            with pytest.raises(hip.RrtmgLwError, match=msg):
                run(cs.with_size(bad, "reliq", col, 61.0))
            _still_the_same(hip, before, (entry, name, "both sizes out"))


@pytest.mark.parametrize("iceflag", [0, 1, 2, 3])
def test_several_violations_in_one_call(hip, oracle, before, iceflag):
    """violations of different kinds in different columns (different 64-column blocks) of one call: the text is one of those present -
    which one is not pinned, the kernels race for the error word by design"""
    d = cs.stop_call(iceflag, 1)
    cloudy = np.nonzero(np.asarray(d["cldfr"])[:, 8] > 0)[0]
    a, b = int(cloudy[0]), int(cloudy[-1])
    assert a // 64 != b // 64
    bad = cs.with_size(cs.with_size(d, "reice", a, 1.0), "reliq", b, 100.0)
    present = {cs.STOPS[s - 1] for s in np.unique(cs.decisions(bad)["stop"]) if s}
    assert len(present) == 2
    for entry, run in _entries(hip, oracle):
        with pytest.raises(hip.RrtmgLwError) as e:
            run(bad)
        assert any(m in str(e.value) for m in present), (entry, str(e.value), present)
        _still_the_same(hip, before, (entry, iceflag))


# ------------------------------------------------------------------------------------------------------------ 5. 256 g-points
@pytest.fixture()
def hip256(hip):
    hip.select_gpoints(256)
    try:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        yield hip
        hip.finalize(selected_only=True)
    finally:
        hip.select_gpoints(140)


def test_g256_families_match_the_oracle(hip256, calls, decs):
    from oracle.bindings import Oracle
    o256 = Oracle(gpoints=256)
    assert hip256.gpoints() == 256
    use = 0.0
    for key, d in calls.items():
        got = hip256.rrtmg_lw_from_dict(d, icld=2, idrv=1)
        use = max(use, _compare_broadband(got, _oracle_gcm(o256, key, d, 2, 1, "256"), 1, d, decs[key], f"256 g-points {key}"))
    print(f"256 g-points, families A and B: bar use {use:.3f}")
