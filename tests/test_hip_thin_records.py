"""k_sweepc takes a shorter body for a quad record whose cell codes are series ("thin", odepth <= 0.06) codes in all 64 lanes of the wave
and the general body - transmittance table and series terms - otherwise.  Which of the two a column's cell goes through therefore
follows from the 63 columns it shares a block with, and the results may not: both bodies round a cell alike
(rrtmg_lw_amd/csrc/kernels.hip, decode_thin).

130 benchmark columns ("cloudy"), of which columns 101 and 129 carry the CO2 and N2O of the "highgas" stress set: block 0 (columns
0-63) is light throughout, block 1 (64-127) has one heavy lane, the ragged last block (128, 129) one light and one heavy column.
Batches this small take the one sweep launch by default, which never runs k_sweepc: the tests switch that off.
"""
import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs, make_stress_inputs

pytestmark = pytest.mark.gpu

NCOL, NLAY = 130, 72
HEAVY = (101, 129)
TOP = 14                                    # the benchmark columns' clouds end at layer 14: above it k_sweepc sweeps, in every mode
NG = (10, 12, 16, 14, 16, 8, 12, 8, 12, 6, 8, 8, 4, 2, 2, 2)      # g-points per band; a band's quads are its g-points in fours
OUTPUTS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
TIGHT_FLUX = 5e-5                           # W m-2 and K d-1: the bars of tests/test_hip_parity.py
TIGHT_HR = 5e-5

_cache = {}


def _inputs():
    if "d" not in _cache:
        d = make_gcm_inputs(NCOL, NLAY, "cloudy", col0=0)
        s = make_stress_inputs("highgas", NCOL, NLAY, col0=0)
        for k in ("co2vmr", "n2ovmr"):
            a = np.array(d[k], order="F")
            for c in HEAVY:
                a[c] = np.asarray(s[k])[c]
            d[k] = a
        _cache["d"] = d
    return _cache["d"]


def _part(d, c0, n):
    p = dict(d)
    p["ncol"] = n
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            p[k] = np.asfortranarray(v[:, c0:c0 + n, :] if (v.ndim == 3 and v.shape[0] == 16) else v[c0:c0 + n])
    return p


@pytest.fixture
def three_launches(hip):
    prev = hip.set_one_sweep_max(0)
    yield hip
    hip.set_one_sweep_max(prev)


def _quads(ngpt):
    """(first g-point, number of g-points) of every quad record, bands in order"""
    assert ngpt == sum(NG)
    q, g0 = [], 0
    for ng in NG:
        q += [(g0 + 4 * i, min(4, ng - 4 * i)) for i in range((ng + 3) // 4)]
        g0 += ng
    return q


def test_premise_the_blocks_differ_in_the_body_they_take(hip):
    """From the gas optical depths (api.gas_optics; the aerosol is zero, odepth = secdiff x taug with 1.50 <= secdiff <= 1.80): a cell is
    certainly thin when 1.80 taug <= 0.06 and certainly thick when 1.50 taug > 0.06.  Above layer 14 there is a (layer, quad) whose record
    is all thin in block 0 and, in block 1, thick in lane 101 and thin in every other lane; and one where, in the ragged block, column 128
    is thin and column 129 thick."""
    d = _inputs()
    assert not np.asarray(d["tauaer"]).any()
    taug = np.asarray(hip.gas_optics(d)["taug"])
    assert taug.shape[:2] == (NCOL, NLAY)
    thin, thick = 1.80 * taug <= 0.06, 1.50 * taug > 0.06
    n_all_thin = n_lane = n_ragged = 0
    for g0, n in _quads(taug.shape[2]):
        for lay in range(TOP, NLAY):
            tn, tk = thin[:, lay, g0:g0 + n].all(axis=1), thick[:, lay, g0:g0 + n].any(axis=1)        # per column
            b0 = tn[:64].all()
            n_all_thin += b0
            others = [c for c in range(64, 128) if c != 101]
            n_lane += b0 and tk[101] and tn[others].all()
            n_ragged += tn[128] and tk[129]
    print(f"records above layer {TOP}: {n_all_thin} all thin in block 0, {n_lane} of them thick in lane 101 alone in block 1; "
          f"{n_ragged} thin in column 128 and thick in column 129")
    assert n_all_thin >= 1 and n_lane >= 1 and n_ragged >= 1


@pytest.mark.parametrize("icld,idrv", [(0, 0), (0, 1), (2, 0), (2, 1)])
def test_a_column_rounds_alike_in_either_body(three_launches, oracle, icld, idrv):
    """The whole call equals, bit for bit, the calls of single columns (a light column alone takes the thin body where, beside a heavy
    neighbour, it took the general one) and of block 1 alone; and it agrees with the oracle at the parity tests' bars."""
    hip, d = three_launches, _inputs()
    full = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    names = OUTPUTS if idrv else OUTPUTS[:6]          # (d(flux)/dT is formed with idrv = 1 only)
    for c0, n in [(3, 1), (100, 1), (101, 1), (102, 1), (128, 1), (129, 1), (64, 64)]:
        got = hip.rrtmg_lw_from_dict(_part(d, c0, n), icld=icld, idrv=idrv)
        for k in names:
            assert np.array_equal(got[k], full[k][c0:c0 + n]), (k, c0, n)
    ref = oracle.rrtmg_lw(NCOL, NLAY, icld, idrv, d)
    dflux = max(np.abs(full[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    dhr = max(np.abs(full[k] - ref[k]).max() for k in ("hr", "hrc"))
    ddt = max(np.abs(full[k] - ref[k]).max() for k in ("duflx_dt", "duflxc_dt")) if idrv else 0.0
    print(f"icld{icld} idrv{idrv}: max|dflux|={dflux:.3e} W/m2  max|dhr|={dhr:.3e} K/d  max|d(dF/dT)|={ddt:.3e}")
    assert np.isfinite(full["uflx"]).all() and np.isfinite(full["hr"]).all()
    assert dflux <= TIGHT_FLUX and dhr <= TIGHT_HR and ddt <= TIGHT_FLUX
