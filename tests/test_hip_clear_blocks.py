"""Block groups of a cloudy call that hold no cloud are swept like a cloud-free call: one k_sweepc<., 0> launch over the whole column, one
stream, 8-byte partials, instead of the three cloudy launches with two identical streams (rrtmg_lw_hip_set_clear_groups; kernels.hip,
SweepArgs::cfree).  Which path a cloud-free 64-column block takes follows from the eleven blocks it shares a sorted group with - that is,
from the batch size and from its neighbours' clouds - and the results may not: every comparison between paths here is bit for bit.

Inputs: 72-layer "cloudy" benchmark columns whose cloud (cldfr, cliqwp, cicewp) is zeroed in whole 64-column blocks.  1 570 columns are
25 blocks, the last of 34 columns.  Batches this small take the one sweep launch by default, which never runs k_sweepc: the tests switch
that off, and the column order too unless they are about it.
"""
import ctypes

import numpy as np
import pytest

from rrtmg_lw_amd.clear_blocks import block_tops, colsort, column_tops, sorted_groups
from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

NCOL, NLAY = 1570, 72
OUTPUTS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
TIGHT_FLUX = 5e-5                           # W m-2, K d-1 and W m-2 K-1: the bars of tests/test_hip_parity.py
TIGHT_HR = 5e-5
# cloud-free blocks of the two layouts (of blocks 0 .. 24; block 24 is the ragged one)
LAYOUTS = {"a": [b for b in range(25) if b % 2 == 1 or b == 24],            # 12 cloudy, 13 cloud-free, interleaved
           "b": [b for b in range(25) if b % 2 == 1 or b >= 22]}            # 11 cloudy, 14 cloud-free

_cache = {}


def _inputs(layout):
    if layout not in _cache:
        if "base" not in _cache:
            _cache["base"] = make_gcm_inputs(NCOL, NLAY, "cloudy", col0=0)
        d = dict(_cache["base"])
        for k in ("cldfr", "cliqwp", "cicewp"):
            a = np.array(d[k], order="F")
            for b in LAYOUTS[layout]:
                a[64 * b:64 * (b + 1)] = 0.0
            d[k] = a
        _cache[layout] = d
    return _cache[layout]


def _part(d, c0, n):
    p = dict(d)
    p["ncol"] = n
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            p[k] = np.asfortranarray(v[:, c0:c0 + n, :] if (v.ndim == 3 and v.shape[0] == 16) else v[c0:c0 + n])
    return p


def _oracle(oracle, layout, icld, idrv):
    key = ("ref", layout, icld, idrv)
    if key not in _cache:
        _cache[key] = oracle.rrtmg_lw(NCOL, NLAY, icld, idrv, _inputs(layout))
    return _cache[key]


def _arrays(out):
    return sorted(k for k, v in out.items() if isinstance(v, np.ndarray))


def _same(a, b, names, tag, sl=slice(None)):
    for k in names:
        assert np.array_equal(a[k], b[k][sl]), (tag, k)


@pytest.fixture
def three_launches(hip):
    """three sweep launches whatever the batch size, columns as they lie, cloud-free groups on; everything put back afterwards"""
    prev_one = hip.set_one_sweep_max(0)
    prev_min = hip.column_sort_min()
    prev_sort = hip.set_column_sort(False, -1)
    prev_cg = hip.set_clear_groups(True)
    try:
        yield hip
    finally:
        hip.set_clear_groups(prev_cg)
        hip.set_column_sort(prev_sort, prev_min)
        hip.set_one_sweep_max(prev_one)
        hip.set_batch(0)


def test_premise_the_layouts_have_the_groups_they_were_designed_for():
    """(a): the sorted groups are {12 cloudy blocks}, {12 cloud-free blocks}, {the ragged cloud-free block}.  (b): the first group holds 11
    cloudy blocks and the cloud-free block 1, which therefore takes the cloudy path; the other two hold no cloud.  At 1 024 columns per batch
    block 1 shares its group with cloudy blocks in both layouts, and a 64-column call of a cloud-free block is a cloud-free group."""
    for layout, nfree in (("a", 13), ("b", 14)):
        d = _inputs(layout)
        bt = block_tops(column_tops(d["cldfr"]))
        assert len(bt) == 25 and sorted(np.flatnonzero(bt == 0)) == LAYOUTS[layout] and len(LAYOUTS[layout]) == nfree
        assert (bt[bt != 0] >= 10).all()                    # (the cloudy blocks' decks reach the benchmark's layer 14 or so)
        groups, hand = sorted_groups(bt)
        assert [len(g) for g in groups] == [12, 12, 1] and hand[1:] == [0, 0] and hand[0] > 0
        assert list(groups[2]) == [24]
        if layout == "a":
            assert (bt[groups[0]] > 0).all() and sorted(groups[1]) == [b for b in range(24) if b % 2 == 1]
        else:
            assert (bt[groups[0][:11]] > 0).all() and groups[0][11] == 1 and (bt[groups[1]] == 0).all()
        g16, h16 = sorted_groups(bt[:16])                   # the first batch of 1 024 columns: 16 blocks
        assert 1 in g16[0] and h16[0] > 0
        for c in ("cliqwp", "cicewp"):
            assert not np.asarray(d[c])[64:128].any()


@pytest.mark.parametrize("layout", ["a", "b"])
@pytest.mark.parametrize("icld,idrv", [(2, 0), (2, 1), (1, 0)])
def test_a_block_rounds_alike_on_either_path(three_launches, oracle, layout, icld, idrv):
    """Switch on against switch off, the whole call against calls of single blocks (a cloud-free block alone is a cloud-free group; inside
    layout (b)'s first group block 1 took the cloudy path) and against batches of 1 024 columns, all bit for bit; and the oracle at the
    parity bars."""
    hip, d = three_launches, _inputs(layout)
    names = OUTPUTS if idrv else OUTPUTS[:6]
    on = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    hip.set_clear_groups(False)
    off = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    hip.set_clear_groups(True)
    _same(on, off, names, "on / off")
    for b in (0, 1, 3, 22, 23, 24):                     # cloudy, cloud-free (in (b) beside cloudy blocks), .., cloudy in (a) only, .., ragged
        c0, n = 64 * b, min(64, NCOL - 64 * b)
        _same(hip.rrtmg_lw_from_dict(_part(d, c0, n), icld=icld, idrv=idrv), on, names, f"block {b} alone", slice(c0, c0 + n))
    hip.set_batch(1024)
    _same(hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv), on, names, "batches of 1 024")
    hip.set_batch(0)
    ref = _oracle(oracle, layout, icld, idrv)
    dflux = max(np.abs(on[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    dhr = max(np.abs(on[k] - ref[k]).max() for k in ("hr", "hrc"))
    ddt = max(np.abs(on[k] - ref[k]).max() for k in ("duflx_dt", "duflxc_dt")) if idrv else 0.0
    print(f"layout ({layout}) icld{icld} idrv{idrv}: max|dflux|={dflux:.3e} W/m2  max|dhr|={dhr:.3e} K/d  max|d(dF/dT)|={ddt:.3e}")
    assert np.isfinite(on["uflx"]).all() and np.isfinite(on["hr"]).all()
    assert dflux <= TIGHT_FLUX and dhr <= TIGHT_HR and ddt <= TIGHT_FLUX
    free = np.concatenate([np.arange(64 * b, min(64 * (b + 1), NCOL)) for b in LAYOUTS[layout]])
    assert np.array_equal(on["uflx"][free], on["uflxc"][free]) and np.array_equal(on["dflx"][free], on["dflxc"][free])
    assert np.abs(on["dflx"] - on["dflxc"]).max() > 1.0           # (and the clouds of the other blocks matter)


@pytest.mark.parametrize("layout", ["a", "b"])
def test_mcica_mask_call(three_launches, oracle, layout):
    """The fused generator + rtrnmc entry (sub-columns as bit masks): a block none of whose columns has cloud has none in any sub-column.
    Alone, a cloud-free block is a cloud-free group; inside layout (b)'s first group block 1 went through k_sweepz<., 4>."""
    hip, d = three_launches, _inputs(layout)
    names = OUTPUTS[:6]
    on = hip.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, icld=2)
    hip.set_clear_groups(False)
    off = hip.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, icld=2)
    hip.set_clear_groups(True)
    _same(on, off, names, "on / off")
    for b in (0, 1, 3, 22, 23, 24):                     # (as in test_a_block_rounds_alike_on_either_path: the kissvec generator seeds a column from its own pressures)
        c0, n = 64 * b, min(64, NCOL - 64 * b)
        _same(hip.rrtmg_lw_mcica_subcol_from_dict(_part(d, c0, n), 140, 0, icld=2), on, names, f"block {b} alone", slice(c0, c0 + n))
    hip.set_batch(1024)
    _same(hip.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, icld=2), on, names, "batches of 1 024")
    hip.set_batch(0)
    sc = oracle.mcica_subcol(NCOL, NLAY, 2, 140, 0, d["play"], d["cldfr"], d["cicewp"], d["cliqwp"], d["reice"], d["reliq"], d["taucld"],
                             np.zeros((NCOL, NLAY)))
    dd = dict(d)
    dd.update({k: sc[k] for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "taucmcl")})
    ref = oracle.rrtmg_lw(NCOL, NLAY, 2, d["idrv"], dd, mcica=True)
    dflux = max(np.abs(on[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    dhr = max(np.abs(on[k] - ref[k]).max() for k in ("hr", "hrc"))
    print(f"layout ({layout}) McICA: max|dflux|={dflux:.3e} W/m2  max|dhr|={dhr:.3e} K/d")
    assert dflux <= TIGHT_FLUX and dhr <= TIGHT_HR


def test_spectral_outputs(three_launches):
    hip, d = three_launches, _inputs("b")
    on = hip.rrtmg_lw_from_dict(d, icld=2, idrv=0, spectral=True)
    hip.set_clear_groups(False)
    off = hip.rrtmg_lw_from_dict(d, icld=2, idrv=0, spectral=True)
    names = _arrays(on)
    assert {"uflxs", "dflxs"} <= set(names) and names == _arrays(off)
    _same(on, off, names, "spectral on / off")


def _launches(hip, d):
    buf = ctypes.create_string_buffer(1 << 16)
    hip.lib().rrtmg_lw_hip_profile_begin()
    hip.rrtmg_lw_from_dict(d, icld=2, idrv=0)
    hip.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
    return [ln.split()[0] for ln in buf.value.decode().splitlines() if ln.strip()]


def test_the_cloudy_call_launches_the_cloud_free_sweep(three_launches):
    hip, d = three_launches, _inputs("a")
    on = _launches(hip, d)
    hip.set_clear_groups(False)
    off = _launches(hip, d)
    p0 = [k for k in on if k.startswith("k_sweepc<") and k.split(",")[1].startswith("0")]
    print("switch on:", sorted(set(k for k in on if k.startswith("k_sweep"))))
    assert len(p0) >= 4                                                         # (one per class of bands with the same number of quads)
    assert any(k.startswith("k_sweepz<") for k in on) and any(k.startswith("k_sweepc<") and k.split(",")[1].startswith("2") for k in on)
    assert not [k for k in off if k.startswith("k_sweepc<") and k.split(",")[1].startswith("0")]
    assert any(k.startswith("k_sweepz<") for k in off)


def test_reordered_windows(three_launches):
    """3 200 plain benchmark columns, every window of 256 reordered by cloud top: the windows' cloud-free columns gather in blocks of their
    own, those blocks in groups of their own."""
    hip = three_launches
    n = 3200
    d = make_gcm_inputs(n, NLAY, "cloudy", col0=0)
    tops = column_tops(d["cldfr"])
    assert (block_tops(tops) > 0).all()                                          # as the columns lie no block is cloud-free
    perm, gains, _ = colsort(tops, NLAY, 0, 0)
    bt = block_tops(tops[perm])
    groups, hand = sorted_groups(bt)
    print(f"{(tops == 0).mean():.3f} of the columns cloud-free; sorted: {(bt == 0).sum()} of {len(bt)} blocks, hand-off levels {hand}")
    assert (bt == 0).sum() >= 2 and hand[-1] == 0 and hand[0] > 0
    plain = hip.rrtmg_lw_from_dict(d, icld=2, idrv=1)
    hip.set_column_sort(True, 0)
    on = hip.rrtmg_lw_from_dict(d, icld=2, idrv=1)
    hip.set_clear_groups(False)
    off = hip.rrtmg_lw_from_dict(d, icld=2, idrv=1)
    _same(on, off, OUTPUTS, "sorted: on / off")
    _same(on, plain, OUTPUTS, "sorted / unsorted")


def test_clear_block_bonus_setter(three_launches):
    hip = three_launches
    d = make_gcm_inputs(1024, NLAY, "cloudy", col0=0)
    plain = hip.rrtmg_lw_from_dict(d, icld=2, idrv=0)
    prev = hip.column_sort_clear()
    try:
        hip.set_column_sort(True, -1)                                            # default threshold, default bonus
        _same(hip.rrtmg_lw_from_dict(d, icld=2, idrv=0), plain, OUTPUTS[:6], "default bonus")
        assert hip.set_column_sort_clear(18) == prev and hip.column_sort_clear() == 18
        _same(hip.rrtmg_lw_from_dict(d, icld=2, idrv=0), plain, OUTPUTS[:6], "bonus 18")
        assert hip.set_column_sort_clear(0) == 18 and hip.column_sort_clear() == 0
    finally:
        hip.set_column_sort_clear(prev)
