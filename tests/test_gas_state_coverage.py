"""The ledger of the designed gas states (tests/gas_states.py) and the CPU half of their parity chain.

Ledger: every branch of setcoef / taumol named in the table below is reached by at least MIN_CELLS (column, layer) cells of the set, in
its shuffled order, and in at least MIN_BLOCKS different blocks of 64 columns - conditions on the design, checked with
gas_states.decisions().  Parity: the oracle is finite on the set, equals the reference's own Fortran on it where that is built, and
equals the committed reference-made fixture tests/golden/ref_gasstate_L52.npz (tools/gen_ref_fixtures.py --gasstate) everywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gas_states as gs  # noqa: E402
from test_hip_spectral import inatm  # noqa: E402
from test_oracle_vs_ref import TOL  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "ref_gasstate_L52.npz")
NLAY, SEED = 52, 0
MIN_CELLS, MIN_BLOCKS = 8, 2
OUT_KEYS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")

# ---- the table -----------------------------------------------------------------------------------------------------------------
# binary bands by region, with the number of mixtures js / jpl / jm can take (specparm is capped below 1: js = 9 / 5 is never reached)
BINARY_BANDS = {"lower": ((3, 4, 5, 7, 9, 12, 13, 15, 16), 8), "upper": ((3, 4, 5), 4)}
MINOR_RATIOS = {(3, "lower"): ("jmn2o",), (3, "upper"): ("jmn2o",), (5, "lower"): ("jmo3",), (7, "lower"): ("jmco2",),
                (9, "lower"): ("jmn2o",), (13, "lower"): ("jmco2", "jmco"), (15, "lower"): ("jmn2",)}
ADJUSTMENTS = {(3, "lower"): 1.5, (3, "upper"): 1.5, (6, "lower"): 3.0, (7, "lower"): 3.0, (7, "upper"): 3.0, (8, "lower"): 3.0,
               (8, "upper"): 3.0, (9, "lower"): 1.5, (9, "upper"): 1.5, (13, "lower"): 3.0}
INDEX_ENDS = {"jp": (1, 58), "jt": (1, 4), "jt1": (1, 4), "indself": (1, 9), "indfor": (1, 2, 3), "indminor": (1, 18), "regime": (0, 1, 2)}
# bands whose first key species is water vapour below laytrop: specparm is exactly 0 where H2O = 0
H2O_FIRST = (3, 4, 5, 7, 9, 12, 13, 16)


def ledger(dec):
    """[(cell name, boolean (ncol, nlay) mask of the atmosphere's cells that reach it)]"""
    rows = []
    for region, (bands, nmix) in BINARY_BANDS.items():
        for band in bands:
            for kind in ("main", "jp1", "planck"):
                sp, js = dec["spec"][(band, region, kind)]
                tag = f"band {band} {region} {kind}"
                rows += [(f"{tag} specparm < 0.125", sp < 0.125), (f"{tag} specparm middle", (sp >= 0.125) & (sp <= 0.875)),
                         (f"{tag} specparm > 0.875", sp > 0.875)]
                rows += [(f"{tag} js = {j}", js == j) for j in range(1, nmix + 1)]
                if kind != "planck":
                    rows += [(f"{tag} just below 0.125", (sp < 0.125) & (sp > 0.124)), (f"{tag} just above 0.125", (sp > 0.125) & (sp < 0.126)),
                             (f"{tag} just below 0.875", (sp < 0.875) & (sp > 0.874)), (f"{tag} just above 0.875", (sp > 0.875) & (sp < 0.876)),
                             (f"{tag} capped at oneminus", sp == gs.ONEMINUS)]
            for kind in MINOR_RATIOS.get((band, region), ()):
                js = dec["spec"][(band, region, kind)][1]
                rows += [(f"band {band} {region} {kind} = {j}", js == j) for j in range(1, nmix + 1)]
    for band in H2O_FIRST:
        rows.append((f"band {band} lower specparm = 0", dec["spec"][(band, "lower", "main")][0] == 0.0))
    for (band, region), thr in ADJUSTMENTS.items():
        ratio, above = dec["adj"][(band, region)]
        inreg = np.isfinite(ratio)
        tag = f"band {band} {region} adjustment"
        rows += [(f"{tag} below", inreg & ~above), (f"{tag} above", above),
                 (f"{tag} within 10 % below", (ratio > 0.9 * thr) & (ratio <= thr)), (f"{tag} within 10 % above", (ratio > thr) & (ratio < 1.1 * thr)),
                 (f"{tag} well beyond", ratio > 2.0 * thr)]
    for k, ends in INDEX_ENDS.items():
        rows += [(f"{k} = {v}", (dec[k] == v) & (dec["lower"] if k == "indself" else True)) for v in ends]
    rows.append(("jp = 1 with fp < 0", (dec["jp"] == 1) & (dec["fp"] < 0)))
    return rows


def counts(dec):
    """[(cell name, number of cells, number of 64-column blocks)]"""
    return [(name, int(m.sum()), int(np.unique(np.nonzero(m.any(axis=1))[0] // 64).size)) for name, m in ledger(dec)]


@pytest.fixture(scope="module")
def states():
    return gs.make_gas_states(NLAY, SEED, "shuffled")


def test_every_ledger_cell_is_reached(states):
    assert 512 <= states["ncol"] <= 1024
    rows = counts(gs.decisions(states))
    assert len(rows) > 600
    short = [r for r in rows if r[1] < MIN_CELLS or r[2] < MIN_BLOCKS]
    assert not short, short


def test_design_values_are_met_exactly(states):
    """the columns are constructed, not drawn: a column built for specparm = s has it, to rounding, in every layer of its region"""
    dec = gs.decisions(states)
    for i, lab in enumerate(states["labels"]):
        if " main s=" not in lab or "clamp" in lab:
            continue
        key, region = lab.split()[0], lab.split()[1]
        s = float(lab.split("s=")[1].split()[0])
        band = {"h2o/co2": 3, "o3/co2": 4, "h2o/o3": 7, "h2o/ch4": 9, "h2o/n2o": 13, "n2o/co2": 15}[key]
        sp = dec["spec"][(band, region, "main")][0][i]
        sp = sp[np.isfinite(sp)]
        # (a first species other than water vapour is never 0: setcoef's floor of 1e-32 coldry leaves specparm ~ 1e-12 / vmr of the second)
        assert sp.size and np.abs(sp - s).max() <= (1e-12 if s > 0 or key.startswith("h2o") else 1e-5), (lab, sp)
    # no exact thresholds: the designed values keep 1e-6 from them, and no ratio that merely follows from a design (another band's, the
    # jp + 1 plane's) comes within 1e-9 - seven decades above the rounding of the quotient that could legitimately pick the other branch
    assert all(1e-6 <= min(abs(s - 0.125), abs(s - 0.875)) <= 1e-3 for s in gs.NEAR)
    for (band, region, kind), (sp, js) in dec["spec"].items():
        sp = sp[np.isfinite(sp)]
        assert (np.minimum(np.abs(sp - 0.125), np.abs(sp - 0.875)) >= 1e-9).all(), (band, region, kind)


def test_orders_and_determinism(states):
    grouped = gs.make_gas_states(NLAY, SEED, "grouped")
    again = gs.make_gas_states(NLAY, SEED, "shuffled")
    perm = states["perm"]
    assert sorted(perm) == list(range(states["ncol"])) and not np.array_equal(perm, np.arange(states["ncol"]))
    for k, v in states.items():
        if isinstance(v, np.ndarray) and k != "perm":
            assert np.array_equal(v, again[k]), k
            assert np.array_equal(v, grouped[k][:, perm] if k == "taucld" else grouped[k][perm]), k
    # grouped: the design points of one stencil branch lie side by side - the first 64-column wave holds only targets below 0.125
    first = [lab.split("s=")[1].split()[0] for lab in grouped["labels"][:64]]
    assert all(s != "clamp" and float(s) < 0.125 for s in first), first
    # shuffled: the layers of a 256-column window span more reference-pressure planes than k_layer's narrow staging window holds
    jp = gs.decisions(states)["jp"]
    assert (jp[:256].max(axis=0) - jp[:256].min(axis=0)).max() >= 4


def test_oracle_is_finite_on_the_designed_set(oracle, states):
    d = states
    for dd in (d, gs.with_clouds(d)):
        o = oracle.rrtmg_lw(d["ncol"], d["nlay"], dd["icld"], 1, dd)
        for k in OUT_KEYS:
            assert np.isfinite(o[k]).all(), k
    for i in range(d["ncol"]):
        c = oracle.column(inatm(d, i, 0))
        assert np.isfinite(c["taug"]).all() and np.isfinite(c["fracs"]).all(), d["labels"][i]


def test_oracle_matches_the_live_reference(oracle, states):
    from oracle.bindings import Reference
    if not Reference.available():
        pytest.skip("oracle/_ref not built (needs the reference sources and flang)")
    ref = Reference()
    d = states
    for dd in (d, gs.with_clouds(d)):
        a = oracle.rrtmg_lw(d["ncol"], d["nlay"], dd["icld"], 1, dd)
        b = ref.rrtmg_lw(d["ncol"], d["nlay"], dd["icld"], 1, dd)
        for k in OUT_KEYS:
            err = np.abs(a[k] - b[k])
            assert err.max() <= TOL, (k, float(err.max()), d["labels"][int(np.argmax(err.max(axis=1)))])
    for i in range(d["ncol"]):
        col = inatm(d, i, 0)
        a, b = oracle.column(col), ref.column(col)
        for k in ("taug", "fracs"):
            assert np.allclose(a[k], b[k], rtol=1e-12, atol=0), (k, d["labels"][i])


def test_oracle_matches_the_committed_reference_fixture(oracle, states):
    f = np.load(FIXTURE)
    assert int(f["nlay"]) == NLAY and int(f["seed"]) == SEED
    cols = f["cols"]
    assert [states["labels"][i] for i in cols] == [str(s) for s in f["labels"]], "the design changed: tools/gen_ref_fixtures.py --gasstate"
    sub = gs.take(states, cols)
    o = oracle.rrtmg_lw(sub["ncol"], NLAY, 0, 1, sub)
    for k in OUT_KEYS:
        assert np.abs(o[k] - f[k]).max() <= TOL, k
    for n, i in enumerate(cols):
        c = oracle.column(inatm(states, int(i), 0))
        for k in ("taug", "fracs"):
            assert np.allclose(c[k][f["lays"][n]], f[k][n], rtol=1e-12, atol=0), (k, states["labels"][i])
