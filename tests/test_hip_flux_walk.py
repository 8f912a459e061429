"""k_flux walks the levels of a chunk per position with the net fluxes of the level below in registers, and exchanges a level's values
through LDS - position -> column - only in the windows k_colsort reordered (kernels.hip: FLUX_CH = 18 levels per chunk).  Which chunk a level
falls in, whether its window was reordered, how many slabs a group has and how the call was cut into batches may not show in any output:
every comparison between paths here is bit for bit, and one path per case is held against the oracle at the bars of
tests/test_hip_clear_blocks.py.

Inputs: 1 570 "cloudy" benchmark columns - 6 full windows of 256 and a ragged one of 34; 24 full 64-column blocks and a partial one -
whose cloud is zeroed in windows 1, 4 and 5: those have nothing to gain from an order, nor has the ragged window, a single block.  With the
threshold lowered to one block-level windows 0, 2 and 3 are reordered and the other four keep their order, so both of k_flux's store paths
run in one launch; with threshold 0 every window counts as reordered and the ragged one takes the exchange as well.  Layer counts 20 and 72 give 21 and 73 levels:
chunks of 18 + 3 and 4 x 18 + 1; 35 layers are two whole chunks.  On the 20- and 35-layer grids the deck lies at the pressures it has on
the 72-layer grid it was written for, not at the same layer indices (_deck_at_its_pressures).  Batches this small take the one sweep launch by default, which asks for
no column order: the tests switch that off.
"""
import numpy as np
import pytest

from rrtmg_lw_amd.clear_blocks import WIN, colsort, column_tops
from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

NCOL = 1570
FLUX_CH = 18                                # kernels.hip
NLAYS = (20, 72, 35)
CLEAR_WINDOWS = (1, 4, 5)
OUTPUTS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
TIGHT_FLUX = 5e-5                           # W m-2, K d-1 and W m-2 K-1: the bars of tests/test_hip_clear_blocks.py
TIGHT_HR = 5e-5
SORT_MIN = 1                                # block-levels: every window with anything to gain is reordered

_cache = {}


CLOUD_ARRAYS = ("cldfr", "cliqwp", "cicewp", "reliq", "reice")
CLOUD_LAYERS = range(5, 14)                 # synth.py: the benchmark's deck, layers 6 .. 14 of ANY grid


def _deck_at_its_pressures(d, nlay):
    """The benchmark's cloud deck is written by layer INDEX for the 72-layer grid, where layers 6 .. 14 lie between 530 and 160 hPa and
    are 18 hPa thick or more.  On the 20-layer grid the same indices are 58 .. 1.2 hPa with layers down to 0.7 hPa thick - cloud water in
    the upper stratosphere - and on 35 layers 200 .. 22 hPa.  The deck is moved to the layers that hold its pressures on this grid (each
    layer 6 .. 14 of the 72-layer grid, bottom to top, to the layer its mid-pressure falls in; a later one replaces an earlier one), with
    each column's draws as they are.  Why it matters for the oracle bars and not only for realism: the heating rate is
    heatfac * (net(l) - net(l+1)) / dp with heatfac = 8.4 K d-1 hPa (W m-2)-1, and the fluxes come from float32 transmittance codes
    (2^-24 of ~400 W m-2 = 2.4e-05 W m-2 per rounding); where cloud decorrelates the errors of a layer's two levels an absolute bar of
    5e-05 K d-1 needs dp of a few hPa at least, which no grid gives the deck at those indices but the one it was written for."""
    ref = make_gcm_inputs(1, 72, "cloudy", col0=0)["plev"][0]
    edges = np.asarray(d["plev"])[0]
    new = {k: np.array(d[k], order="F") for k in CLOUD_ARRAYS}
    clear = make_gcm_inputs(1, nlay, "clear", col0=0)
    for k in CLOUD_ARRAYS:                                  # no deck: the generator's values of a cloud-free layer
        new[k][:, list(CLOUD_LAYERS)] = np.asarray(clear[k])[0, 0]
    for s in CLOUD_LAYERS:
        pmid = 0.5 * (ref[s] + ref[s + 1])
        t = int(np.searchsorted(-edges, -pmid)) - 1         # edges decrease: the layer between edges[t] and edges[t + 1]
        assert 0 <= t < nlay and edges[t] >= pmid >= edges[t + 1]
        for k in CLOUD_ARRAYS:
            new[k][:, t] = np.asarray(d[k])[:, s]
    return new


def _inputs(nlay):
    if nlay not in _cache:
        d = dict(make_gcm_inputs(NCOL, nlay, "cloudy", col0=0))
        if nlay != 72:
            d.update(_deck_at_its_pressures(d, nlay))
        for k in ("cldfr", "cliqwp", "cicewp"):
            a = np.array(d[k], order="F")
            for w in CLEAR_WINDOWS:
                a[WIN * w:WIN * (w + 1)] = 0.0
            d[k] = a
        _cache[nlay] = d
    return _cache[nlay]


def _part(d, c0, n):
    p = dict(d)
    p["ncol"] = n
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            p[k] = np.asfortranarray(v[:, c0:c0 + n, :] if (v.ndim == 3 and v.shape[0] == 16) else v[c0:c0 + n])
    return p


def _oracle(oracle, nlay, icld, idrv):
    key = ("ref", nlay, icld, idrv)
    if key not in _cache:
        _cache[key] = oracle.rrtmg_lw(NCOL, nlay, icld, idrv, _inputs(nlay))
    return _cache[key]


def _same(a, b, names, tag, sl=slice(None)):
    for k in names:
        assert np.array_equal(a[k], b[k][sl]), (tag, k)


@pytest.fixture
def walk(hip):
    """three sweep launches whatever the batch size, windows reordered from one block-level of gain on, cloud-free groups on; everything put
    back afterwards"""
    prev_one = hip.set_one_sweep_max(0)
    prev_min = hip.column_sort_min()
    prev_sort = hip.set_column_sort(True, SORT_MIN)
    prev_cg = hip.set_clear_groups(True)
    try:
        yield hip
    finally:
        hip.set_clear_groups(prev_cg)
        hip.set_column_sort(prev_sort, prev_min)
        hip.set_one_sweep_max(prev_one)
        hip.set_batch(0)


def test_premise_windows_chunks_and_the_split_call():
    """Of the seven windows, 0, 2 and 3 are reordered from one block-level of gain on and 1, 4, 5 and the ragged last one keep their order,
    at every layer count and with any bonus for cloud-free blocks; no gain is negative, so threshold 0 flags every window; the level counts
    are 18 + 3, 4 x 18 + 1 and 2 x 18; a 700-column call is below the default limit of the one-band-per-workgroup sweeps (a slab per band)."""
    for nlay in NLAYS:
        tops = column_tops(_inputs(nlay)["cldfr"])
        for bonus in (0, nlay):
            perm, _, gains = colsort(tops, nlay, SORT_MIN, bonus)
            moved = [bool((perm[w0:w0 + WIN] != np.arange(w0, min(w0 + WIN, NCOL))).any()) for w0 in range(0, NCOL, WIN)]
            assert len(moved) == 7 and [w for w in range(7) if not moved[w]] == sorted(CLEAR_WINDOWS + (6,)), (nlay, bonus, gains)
            assert all((g >= SORT_MIN) == m for g, m in zip(gains, moved)) and min(gains) >= 0
    assert [(n + 1) % FLUX_CH for n in NLAYS] == [3, 1, 0]
    assert 700 <= 768 and 700 % WIN != 0                     # driver.hip: g_split_max; two windows and a ragged one


@pytest.mark.parametrize("nlay", NLAYS)
@pytest.mark.parametrize("icld,idrv", [(0, 0), (0, 1), (2, 0), (2, 1)])
def test_every_path_gives_the_same_bits(walk, oracle, nlay, icld, idrv):
    """Column order on (windows 0, 2, 3 reordered, the others not) against every window reordered and against off, cloud-free groups on against off, batches of 1 024 against one batch,
    the first 700 columns alone (a slab per band: the loop over groups and slabs) and windows 0, 3 and the ragged last one alone, all bit
    for bit; and the oracle at the parity bars (measured: max |dflux| 5.0e-06 .. 7.1e-06 W/m2, max |dhr| 1.3e-06 .. 1.6e-06 K/d over the
    twelve cases; with the deck left at layer indices 6 .. 14 of the 20-layer grid - _deck_at_its_pressures - the two icld 2 cases gave
    5.566e-05 K/d, with the library of the commit before this kernel as with this one)."""
    hip, d = walk, _inputs(nlay)
    names = OUTPUTS if idrv else OUTPUTS[:6]
    run = lambda x=d: hip.rrtmg_lw_from_dict(x, icld=icld, idrv=idrv)
    base = run()
    hip.set_column_sort(True, 0)
    _same(run(), base, names, "every window reordered")
    hip.set_column_sort(False, -1)
    _same(run(), base, names, "column order off")
    hip.set_clear_groups(False)
    _same(run(), base, names, "column order off, cloud-free groups off")
    hip.set_column_sort(True, SORT_MIN)
    _same(run(), base, names, "cloud-free groups off")
    hip.set_clear_groups(True)
    hip.set_batch(1024)
    _same(run(), base, names, "batches of 1 024")
    hip.set_batch(0)
    _same(run(_part(d, 0, 700)), base, names, "700 columns, a slab per band", slice(0, 700))
    for w in (0, 3, 6):
        c0, n = WIN * w, min(WIN, NCOL - WIN * w)
        _same(run(_part(d, c0, n)), base, names, f"window {w} alone", slice(c0, c0 + n))
    ref = _oracle(oracle, nlay, icld, idrv)
    dflux = max(np.abs(base[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    dhr = max(np.abs(base[k] - ref[k]).max() for k in ("hr", "hrc"))
    ddt = max(np.abs(base[k] - ref[k]).max() for k in ("duflx_dt", "duflxc_dt")) if idrv else 0.0
    print(f"nlay {nlay} icld{icld} idrv{idrv}: max|dflux|={dflux:.3e} W/m2  max|dhr|={dhr:.3e} K/d  max|d(dF/dT)|={ddt:.3e}")
    assert dflux <= TIGHT_FLUX and dhr <= TIGHT_HR and ddt <= TIGHT_FLUX
    if icld:
        assert np.abs(base["dflx"] - base["dflxc"]).max() > 1.0          # (the clouds of the other windows matter)
        free = np.concatenate([np.arange(WIN * w, WIN * (w + 1)) for w in CLEAR_WINDOWS])
        assert np.array_equal(base["uflx"][free], base["uflxc"][free]) and np.array_equal(base["dflx"][free], base["dflxc"][free])


@pytest.mark.parametrize("nlay", NLAYS)
def test_every_element_is_written_once_and_nothing_beside(walk, nlay):
    """Device-resident call into outputs pre-filled with NaN, each array between two stamped guard rows: every element comes back finite
    and the guards keep their stamp.  With batches of 768 columns the caller's arrays have a larger leading dimension (1 570) than the
    columns k_flux is given (768, 768 and a ragged 34 from column 1 536): a store past a batch's last column would land in a row an
    earlier batch has written, so the batched call must also equal the unbatched one bit for bit."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    hip = walk
    dev = torch.device("cuda", 0)
    dn = _inputs(nlay)
    d = dict(dn)
    for k, v in dn.items():                 # the host arrays on the device, first index fastest
        if isinstance(v, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(v.transpose())).to(dev)
            d[k] = t.permute(*reversed(range(t.dim())))
    idrv, rows = 1, output_rows(nlay, 1)
    stream = torch.cuda.current_stream().cuda_stream
    got = []
    for batch in (0, 768):
        hip.set_batch(batch)
        buf = torch.full((rows + 2, NCOL), float("nan"), dtype=torch.float64, device=dev)
        hip.rrtmg_lw_device(d, output_views(buf[1:-1], nlay, idrv), icld=2, idrv=idrv, stream=stream)
        hip.check(stream)
        assert bool(torch.isfinite(buf[1:-1]).all()), f"batch {batch}: an element was not written"
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), f"batch {batch}: a guard row was written"
        got.append(buf[1:-1].clone())
    hip.set_batch(0)
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64))
    host = hip.rrtmg_lw_from_dict(dn, icld=2, idrv=idrv)
    dev_out = {k: v.T.cpu().numpy() for k, v in output_views(got[0], nlay, idrv).items()}
    _same(dev_out, host, OUTPUTS, "device entry / host entry")
