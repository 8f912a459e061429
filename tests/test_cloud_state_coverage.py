"""The ledgers of the designed cloud states (tests/cloud_states.py) and the CPU half of their parity chain.

Reach ledger: every (table, interval), clamp, bound and arm of cldprop named in ledger() is reached by at least MIN_CELLS (column, layer)
cells in at least MIN_BLOCKS different 64-column blocks (a block is 64 consecutive columns of one call), every band-count transition
and every inflag likewise - conditions on the design, checked with cloud_states.decisions().

Sensitivity ledger: what makes the GPU comparison (tests/test_hip_cloud_states.py) able to fail.  For every family-A column the particle
size is moved half a table interval and the oracle's per-band fluxes are taken again; the response of a (table, interval, band) cell is
the largest flux change over the columns that read the interval - the GPU test compares EVERY such column at BAND_TOL, so an error in the
cell shows as soon as one of them moves by more than the bar.  The response has to be 4 x BAND_TOL; at most SHORT_CAP of a table's cells
may fall short, and each is named.

Parity: the oracle is finite on families A - C, equals the reference's own Fortran where that is built (non-McICA and McICA), equals the
committed reference-made fixture tests/golden/ref_cloudstate_L40.npz (tools/gen_ref_fixtures.py --cloudstate), gives bit-equal results
with and without the unread out-of-bounds sizes of family C, and stops where - and with the text with which - the reference stops
(family D: the reference itself is never run there, its `stop` ends the process).

`python tests/test_cloud_state_coverage.py` prints the ledgers as the tables of profiles/cloud_state_coverage.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # (under pytest the conftest has put the repository root on the path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cloud_states as cs  # noqa: E402
from test_hip_spectral import BAND_TOL, inatm  # noqa: E402
from test_oracle_vs_ref import TOL  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "ref_cloudstate_L40.npz")
MIN_CELLS, MIN_BLOCKS = 3, 2
MIN_RESPONSE = 4 * BAND_TOL          # 2e-4 W m-2
SHORT_CAP = 0.02
OUT_KEYS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
FLUX_KEYS = ("totuflux", "totdflux", "totuclfl", "totdclfl")
FIXTURE_KEYS = ("uflx", "dflx", "hr")
FIXTURE_STRIDE = 31                  # every 31st column of every call of families A and B


@pytest.fixture(scope="module")
def fam_a():
    return cs.family_a()


@pytest.fixture(scope="module")
def fam_b():
    return cs.family_b()


@pytest.fixture(scope="module")
def fam_c():
    return cs.family_c()


# ------------------------------------------------------------------------------------------------------------------ reach ledger
def ledger(calls):
    """[(cell name, {call key: boolean (ncol, nlay) mask of the cells that reach it})] over the calls {key: dict} of families A and B"""
    rows = {}

    def add(name, key, mask):
        rows.setdefault(name, {})[key] = mask

    for key, d in calls.items():
        dec = cs.decisions(d)
        inflag, iceflag, liqflag = int(d["inflglw"]), int(d["iceflglw"]), int(d["liqflglw"])
        hit = dec["enters"] & dec["cloudy"]                 # cells whose optical depth reaches the sweeps
        rei, rel = np.asarray(d["reice"]), np.asarray(d["reliq"])
        ice, liq = hit & dec["ice_read"], hit & dec["liq_read"]
        tab = "absice%d" % iceflag
        t = cs.TABLES[tab]
        if inflag == 2:
            for k in range(1, t["nint"] + 1):
                add(f"{tab} interval {k}", key, ice & (dec["index_i"] == k))
            if t["nint"]:
                add(f"{tab} clamp index {t['nint'] + 1} -> {t['nint']}", key, ice & (rei == t["hi"]))
                add(f"{tab} fint 0 (node)", key, ice & (dec["fint_i"] == 0.0))
                add(f"{tab} fint 0.25", key, ice & (dec["fint_i"] == 0.25))
            add(f"{tab} lower bound {t['lo']}", key, ice & (rei == t["lo"]))
            add(f"{tab} one ulp above the lower bound", key, ice & (rei == np.nextafter(t["lo"], np.inf)))
            if t["hi"] is not None:
                add(f"{tab} upper bound {t['hi']}", key, ice & (rei == t["hi"]))
                add(f"{tab} one ulp below the upper bound", key, ice & (rei == np.nextafter(t["hi"], -np.inf)))
            if liqflag == 1:
                for k in range(1, 58):
                    add(f"absliq1 interval {k}", key, liq & (dec["index_l"] == k))
                add("absliq1 clamp index 58 -> 57", key, liq & (rel >= 59.5))
                add("absliq1 fint 1.5 (reliq 60)", key, liq & (dec["fint_l"] == 1.5))
                add("absliq1 fint 1.25 (reliq 59.75)", key, liq & (dec["fint_l"] == 1.25))
                add("absliq1 fint 0.25", key, liq & (dec["fint_l"] == 0.25))
                add("absliq1 lower bound 2.5", key, liq & (rel == 2.5))
                add("absliq1 one ulp above the lower bound", key, liq & (rel == np.nextafter(2.5, np.inf)))
                add("absliq1 upper bound 60.0", key, liq & (rel == 60.0))
                add("absliq1 one ulp below the upper bound", key, liq & (rel == np.nextafter(60.0, -np.inf)))
            two = hit
            add(f"arm ciwp == 0, iceflag {iceflag}", key, two & (np.asarray(d["cicewp"]) == 0.0))
            add(f"arm clwp == 0, liqflag {liqflag}", key, two & (np.asarray(d["cliqwp"]) == 0.0))
            add(f"arm mixed, flags {iceflag} / {liqflag}", key, two & dec["ice_read"] & (np.asarray(d["cliqwp"]) != 0.0))
            if iceflag == 1:
                add("iceind 1 -> 2 under clwp == 0", key, two & (dec["promoted"] == 1))
                if liqflag == 0:
                    add("iceind 1 -> 2 under liqflag 0", key, two & (dec["promoted"] == 2))
                else:
                    add("iceind 1 kept (five ice bands in a 16-band layer)", key, two & (dec["iceind"] == 1))
        if d["family"] == "B":
            for a, b in ((1, 1), (5, 5), (16, 16), (1, 16), (1, 5), (5, 16), (16, 5)):
                add(f"band count {a} at the layer -> {b} at the end", key, hit & (dec["nb_at"] == a) & (dec["nb_final"] == b))
            add(f"inflag {inflag}", key, hit)
            cf = np.asarray(d["cldfr"])
            add("fraction 1e-10: enters cldprop, cloud-free for the sweeps", key, dec["enters"] & ~dec["cloudy"] & (cf == cs.TINY))
            add("fraction 1e-21: does not enter", key, ~dec["enters"] & (cf == cs.NOT_ENTERING))
            add("cloudy for the sweeps, does not enter (no water, no optical depth)", key, dec["cloudy"] & ~dec["enters"])
            tiny = (np.asarray(d["cicewp"]) + np.asarray(d["cliqwp"]) == 1.e-25)
            add("water path 1e-25, tauctot above 1e-20: enters", key, tiny & dec["enters"])
            add("water path 1e-25, tauctot below 1e-20: does not enter", key, tiny & ~dec["enters"])
    return list(rows.items())


def counts(calls):
    """[(cell name, number of cells, number of 64-column blocks)]"""
    out = []
    for name, masks in ledger(calls):
        cells = sum(int(m.sum()) for m in masks.values())
        blocks = sum(int(np.unique(np.nonzero(m.any(axis=1))[0] // 64).size) for m in masks.values())
        out.append((name, cells, blocks))
    return out


def _all_calls(fam_a, fam_b):
    calls = {("A",) + k: v for k, v in fam_a.items()}
    calls.update({("B",) + k: v for k, v in fam_b.items()})
    return calls


def test_every_ledger_cell_is_reached(fam_a, fam_b):
    rows = counts(_all_calls(fam_a, fam_b))
    names = [r[0] for r in rows]
    assert sum(n.startswith("absice2 interval") for n in names) == 42 and sum(n.startswith("absice3 interval") for n in names) == 45
    assert sum(n.startswith("absliq1 interval") for n in names) == 57 and len(rows) > 200
    short = [r for r in rows if r[1] < MIN_CELLS or r[2] < MIN_BLOCKS]
    assert not short, short


def test_the_design_is_what_it_says(fam_a, fam_b, fam_c):
    """shapes, determinism, no NaN / Inf, a median optical depth of 0.5 in every family-A cloud, mixed families inside the blocks"""
    again = cs.family_a()
    for key, d in fam_a.items():
        assert d["nlay"] == 40 and d["ncol"] % 64 and d["ncol"] <= 512
        for k, v in d.items():
            if isinstance(v, np.ndarray):
                assert np.isfinite(v).all(), (key, k)
                assert np.array_equal(v, again[key][k]), (key, k)
        assert not np.array_equal(d["perm"], np.arange(d["ncol"]))
        assert not cs.decisions(d)["stop"].any()
        iceflag, liqflag = key
        for i, m in enumerate(d["meta"]):
            if m["kind"] != "table":
                continue
            l = m["lay"]
            tau = d["cicewp"][i, l] * cs.ice_coef(iceflag, d["reice"][i, l]) + d["cliqwp"][i, l] * cs.liq_coef(liqflag, d["reliq"][i, l])
            assert abs(np.median(tau) - cs.TARGET_TAU) <= 1e-12, d["labels"][i]
            assert (d["cicewp"][i, l] == 0.0) == (m["phase"] == "liq") and (d["cliqwp"][i, l] == 0.0) == (m["phase"] == "ice")
        if d["ncol"] > 64:       # the first block holds every height, fraction and phase
            first = [m for m in d["meta"][:64] if m["kind"] == "table"]
            assert {m["lay"] for m in first} == set(cs.HEIGHTS) and {m["cf"] for m in first} == set(cs.FRACTIONS)
            assert len({m["phase"] for m in first}) >= 2
    for key, d in fam_b.items():
        assert d["ncol"] % 64 and d["ncol"] > 64 and not cs.decisions(d)["stop"].any()
        assert all(np.isfinite(v).all() for v in d.values() if isinstance(v, np.ndarray))
    for key, (clean, junk) in fam_c.items():
        assert clean["ncol"] > 256 and clean["ncol"] % 64
        dc, dj = cs.decisions(clean), cs.decisions(junk)
        assert all(np.array_equal(dc[k], dj[k]) for k in dc) and not dj["stop"].any()
        for k in ("reice", "reliq"):
            moved = np.asarray(junk[k])[np.asarray(junk[k]) != np.asarray(clean[k])]
            assert moved.size and set(np.unique(moved)) <= set(cs.JUNK)


# ------------------------------------------------------------------------------------------------------------------ sensitivity ledger
def band_runs(oracle, d, i, icld=2):
    """{band: the oracle's fluxes of that band alone} for column i (band 16 in the broadband call's convention)"""
    col = inatm(d, i, icld)
    r = {b: oracle.column(col, b, b, iout=99) for b in range(1, 16)}
    both = oracle.column(col, 15, 16, iout=99)
    r[16] = {k: both[k] - r[15][k] for k in FLUX_KEYS}
    return r


def sensitivity(oracle, fam_a):
    """{table: (nint, 16) array}: per (interval, band) the largest change of a total-sky band flux, over the family-A columns that read
    the interval, when the column's particle size moves half an interval (towards the inside of the table at its upper end)"""
    resp = {t: np.zeros((cs.TABLES[t]["nint"], 16)) for t in ("absice2", "absice3", "absliq1")}
    for key, d in fam_a.items():
        dec = cs.decisions(d)
        for i, m in enumerate(d["meta"]):
            if m["kind"] != "table" or m["table"] not in resp:
                continue
            t = cs.TABLES[m["table"]]
            rkey, ikey = ("reice", "index_i") if t["phase"] == "ice" else ("reliq", "index_l")
            half = 0.5 * t["step"]
            r = d[rkey][i, m["lay"]]
            moved = cs.with_size(d, rkey, i, r + half if r + half <= t["hi"] else r - half, lay=m["lay"])
            a, b = band_runs(oracle, d, i), band_runs(oracle, moved, i)
            k = int(dec[ikey][i, m["lay"]]) - 1
            for band in range(1, 17):
                delta = max(np.abs(a[band][s] - b[band][s]).max() for s in ("totuflux", "totdflux"))
                resp[m["table"]][k, band - 1] = max(resp[m["table"]][k, band - 1], delta)
    return resp


def short_falls(resp):
    return {t: [(int(k) + 1, int(b) + 1, float(r[k, b])) for k, b in zip(*np.nonzero(r < MIN_RESPONSE))] for t, r in resp.items()}


def test_every_table_cell_moves_a_band_flux_by_four_times_the_bar(oracle, fam_a):
    resp = sensitivity(oracle, fam_a)
    for t, short in short_falls(resp).items():
        print(f"{t}: {len(short)} of {resp[t].size} (interval, band) cells below {MIN_RESPONSE:g} W m-2: {short}")
        print(f"{t}: weakest response per band " + " ".join(f"{v:.2e}" for v in resp[t].min(axis=0)))
        assert len(short) <= SHORT_CAP * resp[t].size, (t, short)


# ------------------------------------------------------------------------------------------------------------------ parity on the CPU
def test_oracle_is_finite_on_families_a_to_c(oracle, fam_a, fam_b, fam_c):
    calls = list(_all_calls(fam_a, fam_b).items()) + [(("C",) + k, v[1]) for k, v in fam_c.items()]
    for key, d in calls:
        for icld in (1, 2):
            o = oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, 1, d)
            for k in OUT_KEYS:
                assert np.isfinite(o[k]).all(), (key, icld, k)
        if key[0] == "A":           # the clouds matter: every column of the walk differs from clear sky
            cloudy = np.array([m["kind"] == "table" for m in d["meta"]])
            assert (np.abs(o["dflx"] - o["dflxc"]).max(axis=1)[cloudy] > 0.1).all(), key


def subcolumns(oracle, d, icld, seed=140):
    sc = oracle.mcica_subcol(d["ncol"], d["nlay"], icld, seed, 0, d["play"], d["cldfr"], d["cicewp"], d["cliqwp"], d["reice"], d["reliq"],
                             d["taucld"], np.zeros((d["ncol"], d["nlay"])))
    dd = dict(d)
    dd.update({k: sc[k] for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "taucmcl")})
    return dd


def test_oracle_matches_the_live_reference(oracle, fam_a, fam_b):
    from oracle.bindings import Reference
    if not (Reference.available() and Reference.available("mcica")):
        pytest.skip("oracle/_ref not built (needs the reference sources and flang)")
    ref, refm = Reference(), Reference("mcica")
    for key, d in _all_calls(fam_a, fam_b).items():
        for icld in (1, 2):
            a, b = oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, 1, d), ref.rrtmg_lw(d["ncol"], d["nlay"], icld, 1, d)
            for k in OUT_KEYS:
                err = np.abs(a[k] - b[k])
                assert err.max() <= TOL, (key, icld, k, float(err.max()), d["labels"][int(np.argmax(err.max(axis=1)))])
        if d["inflglw"] == 1:       # not available with McICA
            continue
        dd = subcolumns(oracle, d, 2)
        a, b = oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 1, dd, mcica=True), refm.rrtmg_lw(d["ncol"], d["nlay"], 2, 1, dd)
        for k in OUT_KEYS:
            err = np.abs(a[k] - b[k])
            assert err.max() <= TOL, ("mcica", key, k, float(err.max()), d["labels"][int(np.argmax(err.max(axis=1)))])


def fixture_columns(calls):
    """[(call key, column indices)]: every FIXTURE_STRIDE-th column of every call, in the order of the calls"""
    return [(key, np.arange(key[1] % 7, d["ncol"], FIXTURE_STRIDE)) for key, d in calls.items()]


def fixture_reference(f, calls):
    """{call key: (columns, {output: array})} of the committed fixture; fails when the design no longer is the one it was made from"""
    res, at = {}, 0
    labels = [str(s) for s in f["labels"]]
    for key, cols in fixture_columns(calls):
        n = len(cols)
        assert labels[at:at + n] == [calls[key]["labels"][i] for i in cols], "the design changed: tools/gen_ref_fixtures.py --cloudstate"
        res[key] = (cols, {k: f[k][at:at + n] for k in FIXTURE_KEYS})
        at += n
    assert at == len(labels)
    return res


def test_oracle_matches_the_committed_reference_fixture(oracle, fam_a, fam_b):
    f = np.load(FIXTURE)
    assert int(f["nlay"]) == cs.NLAY and int(f["seed"]) == cs.SEED and int(f["icld"]) == 2
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(G, "ref_gasstate_L52.npz"))
    calls = _all_calls(fam_a, fam_b)
    for key, (cols, ref) in fixture_reference(f, calls).items():
        sub = cs.take(calls[key], cols)
        o = oracle.rrtmg_lw(sub["ncol"], sub["nlay"], 2, 0, sub)
        for k in FIXTURE_KEYS:
            assert np.abs(o[k] - ref[k]).max() <= TOL, (key, k)


def test_unread_sizes_change_nothing_in_the_oracle(oracle, fam_c):
    for key, (clean, junk) in fam_c.items():
        for icld in (1, 2):
            a, b = (oracle.rrtmg_lw(d["ncol"], d["nlay"], icld, 1, d) for d in (clean, junk))
            for k in OUT_KEYS:
                assert np.array_equal(a[k], b[k]), (key, icld, k)
        if key[0] == 1:
            continue
        da = subcolumns(oracle, clean, 2)
        db = dict(da, reicmcl=np.asfortranarray(junk["reice"]), relqmcl=np.asfortranarray(junk["reliq"]))
        a, b = (oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 1, d, mcica=True) for d in (da, db))
        for k in OUT_KEYS:
            assert np.array_equal(a[k], b[k]), ("mcica", key, k)


@pytest.mark.parametrize("case", cs.stop_cases(), ids=lambda c: c[0] + " iceflag %d" % c[1][0])
def test_oracle_stops_where_the_reference_stops(oracle, case):
    """src/rrtmg_lw_cldprop.f90:212-273 / src/rrtmg_lw_cldprmc.f90:204-254: strict comparisons, so the bound passes and the next double
    beyond it stops; the ice block comes before the liquid block, so a layer with both sizes out stops with the ice text"""
    name, (iceflag, liqflag), phase, key, bound, beyond, msg = case
    d = cs.stop_call(iceflag, liqflag)
    col = cs.first_cloudy_column(d)
    ok, bad = cs.with_size(d, key, col, bound), cs.with_size(d, key, col, beyond)
    assert not cs.decisions(ok)["stop"].any() and cs.STOPS[cs.decisions(bad)["stop"][col, 8] - 1] == msg
    oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 0, ok)
    with pytest.raises(RuntimeError, match=msg):
        oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 0, bad)
    oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 0, subcolumns(oracle, ok, 2), mcica=True)
    with pytest.raises(RuntimeError, match=msg):
        oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 0, subcolumns(oracle, bad, 2), mcica=True)
    if phase == "ice":          # the liquid size out as well, in the same layer: the ice text
        both = cs.with_size(bad, "reliq", col, 61.0)
        for dd, mc in ((both, False), (subcolumns(oracle, both, 2), True)):
            with pytest.raises(RuntimeError, match=msg):
                oracle.rrtmg_lw(d["ncol"], d["nlay"], 2, 0, dd, mcica=mc)


if __name__ == "__main__":
    from oracle.bindings import Oracle
    A, B = cs.family_a(), cs.family_b()
    rows = counts(_all_calls(A, B))
    print("| cell | cells | 64-column blocks |\n|---|---|---|")
    for name, cells, blocks in rows:
        print(f"| {name} | {cells} | {blocks} |")
    resp = sensitivity(Oracle(), A)
    for t, short in short_falls(resp).items():
        print(f"\n{t}: {len(short)} of {resp[t].size} cells below {MIN_RESPONSE:g} W m-2 (cap {SHORT_CAP * resp[t].size:.0f}):",
              ", ".join(f"interval {k} band {b}: {v:.2e}" for k, b, v in short) or "none")
        print("| band | " + " | ".join(str(b) for b in range(1, 17)) + " |\n|" + "---|" * 17)
        print("| weakest response | " + " | ".join(f"{v:.1e}" for v in resp[t].min(axis=0)) + " |")
        print("| median response | " + " | ".join(f"{v:.1e}" for v in np.median(resp[t], axis=0)) + " |")
