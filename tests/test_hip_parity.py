"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Tolerances are the north-star bars of BASELINE.json: |dflux| <= 0.01 W m-2, |dhr| <= 0.001 K/day (and
|d(dF/dT)| <= 0.01 W m-2 K-1); a much tighter "regression" bar (1e-6 relative to the flux scale) is asserted as
well: both sides compute in float64 from the same tables and differ only by FMA contraction, libm vs ocml
exp/log/pow and summation order across band chunks - but a last-bit difference in an optical depth can move the
reference's 1e-4-quantised transmittance look-up (src/rrtmg_lw_rtrn.f90:445-451) to the neighbouring table entry,
which is worth ~1e-6 W m-2; the tight bar is therefore 5e-5, not 1e-12.
"""
import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

FLUX_TOL = 0.01      # W m-2     (BASELINE.json north_star)
HR_TOL = 0.001       # K day-1
TIGHT_FLUX = 5e-5
TIGHT_HR = 5e-5


def _compare(got, ref, idrv, tag):
    dflux = max(np.abs(got[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    dhr = max(np.abs(got[k] - ref[k]).max() for k in ("hr", "hrc"))
    ddt = 0.0
    if idrv == 1:
        ddt = max(np.abs(got[k] - ref[k]).max() for k in ("duflx_dt", "duflxc_dt"))
    print(f"{tag}: max|dflux|={dflux:.3e} W/m2  max|dhr|={dhr:.3e} K/d  max|d(dF/dT)|={ddt:.3e}")
    assert np.isfinite(got["uflx"]).all() and np.isfinite(got["hr"]).all()
    assert dflux <= FLUX_TOL and dhr <= HR_TOL and ddt <= FLUX_TOL
    assert dflux <= TIGHT_FLUX and dhr <= TIGHT_HR and ddt <= TIGHT_FLUX
    assert got["icld"] == ref["icld"]


@pytest.mark.parametrize("config,nlay,icld,ncol", [
    ("clear", 72, 0, 300),      # BASELINE config 2 (replicated MLS columns), reduced column count
    ("clear", 51, 1, 70),       # icld=1 routes a cloud-free call through rtrn
    ("cloudy", 72, 2, 400),     # config 3: maximum-random overlap (rtrnmr)
    ("cloudy", 72, 1, 400),     # random overlap (rtrn)
    ("cloudy", 72, 3, 130),     # icld=3 also takes rtrnmr in the non-McICA build
    ("cloudy", 72, 9, 65),      # out-of-range icld is reset to 2
    ("aer_idrv", 137, 2, 200),  # config 5: aerosol + dF/dT at 137 layers
    ("aer_idrv", 72, 1, 100),
    ("aer_idrv", 33, 0, 64),    # clear call with aerosol and idrv
])
def test_gcm_entry_matches_oracle(hip, oracle, config, nlay, icld, ncol):
    d = make_gcm_inputs(ncol, nlay, config, col0=1000)
    got = hip.rrtmg_lw_from_dict(d, icld=icld)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, d["idrv"], d)
    _compare(got, ref, d["idrv"], f"{config} L{nlay} icld{icld}")


def test_batching_is_transparent(hip, oracle):
    """Results must not depend on how the driver splits the columns into batches."""
    d = make_gcm_inputs(700, 72, "cloudy", col0=5)
    hip.set_batch(131072)
    try:
        one = hip.rrtmg_lw_from_dict(d)
        hip.set_batch(256)
        many = hip.rrtmg_lw_from_dict(d)
    finally:
        hip.set_batch(0)
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
        assert np.array_equal(one[k], many[k]), k


def test_arrays_side_by_side_in_memory_some_of_them_pinned(hip, oracle):
    """Input arrays carved one behind the other from a single allocation, so that neighbours share memory pages, every other one pinned:
    an array between two pinned neighbours is NOT pinned (the runtime's pointer attributes would say so at both of its ends - registrations
    are page-granular - and a direct copy from it faulted on its middle pages); results equal the call with separate arrays."""
    ncol, nlay = 3000, 40
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=13)
    keys = [k for k, v in d.items() if isinstance(v, np.ndarray) and v.dtype == np.float64]
    total = sum(d[k].size for k in keys) + len(keys)
    pool = np.zeros(total + 8)
    packed, pos = dict(d), 3                                  # (3 doubles in: nothing page-aligned)
    for k in keys:
        n = d[k].size
        view = pool[pos:pos + n].reshape(d[k].shape, order="F")
        view[...] = d[k]
        assert view.flags.f_contiguous
        packed[k] = view
        pos += n + 1
    want = hip.rrtmg_lw_from_dict(d)
    pinned = keys[::2]
    for k in pinned:
        hip.host_register(packed[k])
    try:
        for k in keys:
            assert hip.host_is_registered(packed[k]) == (k in pinned), k
        got = hip.rrtmg_lw_from_dict(packed)
    finally:
        for k in pinned:
            hip.host_unregister(packed[k])
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
        assert np.array_equal(got[k], want[k]), k
    assert not hip.host_is_registered(packed[pinned[0]])


def test_a_column_does_not_depend_on_its_neighbours(hip):
    """A column's results - d(flux)/dT included - are the same, bit for bit, whether it is solved alone, in a block of other columns or in
    the whole call: the hand-off level between the clear-sky and the cloud-zone sweeps follows from the clouds of the 64-column block a
    column happens to share, and no level's sum may round differently for it (found by tools/soak_host_entry.py: a product fused into the
    sum over the g-points in one copy of the level body and not in another)."""
    ncol, nlay = 1500, 60
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=7)
    assert d["idrv"] == 1
    full = hip.rrtmg_lw_from_dict(d, icld=2)
    names = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")

    def part(c0, n):
        p = dict(d); p["ncol"] = n
        for k, v in d.items():
            if isinstance(v, np.ndarray):
                p[k] = np.asfortranarray(v[:, c0:c0 + n, :] if (v.ndim == 3 and v.shape[0] == 16) else v[c0:c0 + n])
        return hip.rrtmg_lw_from_dict(p, icld=2)

    cf = np.asarray(d["cldfr"])
    tops = np.array([(np.nonzero(cf[i] > 0)[0] + 1).max() if (cf[i] > 0).any() else 0 for i in range(ncol)])
    assert len(set(tops[:640])) >= 3            # the blocks mix cloud tops (and cloud-free columns)
    for c0, n in [(c, 1) for c in range(0, 640, 37)] + [(5, 3), (100, 64), (131, 65), (700, 257)]:
        got = part(c0, n)
        for k in names:
            assert np.array_equal(got[k], full[k][c0:c0 + n]), (k, c0, n)


def test_cloud_inputs_ignored_when_icld0(hip, oracle):
    """inatm copies cloud arrays only when icld >= 1 (src/rrtmg_lw_rad.nomcica.f90:893-910)."""
    d = make_gcm_inputs(100, 72, "cloudy")
    got = hip.rrtmg_lw_from_dict(d, icld=0)
    ref = oracle.rrtmg_lw(100, 72, 0, 0, d)
    _compare(got, ref, 0, "cloudy inputs, icld=0")
    assert np.array_equal(got["uflx"], got["uflxc"])


def test_physics_error_is_reported(hip):
    """The reference `stop`s on out-of-range particle sizes (src/rrtmg_lw_cldprop.f90:244); the C ABI returns a code."""
    d = make_gcm_inputs(64, 72, "cloudy")
    d["reice"] = np.asfortranarray(np.full((64, 72), 500.0))
    with pytest.raises(hip.RrtmgLwError, match="ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS"):
        hip.rrtmg_lw_from_dict(d)
    # and the library stays usable afterwards
    d = make_gcm_inputs(64, 72, "clear")
    hip.rrtmg_lw_from_dict(d)


@pytest.mark.parametrize("iceflag,liqflag,inflag", [(0, 0, 2), (1, 1, 2), (2, 1, 2), (3, 0, 2), (1, 0, 2), (0, 0, 0), (0, 0, 1)])
def test_cloud_property_options(hip, oracle, iceflag, liqflag, inflag):
    """Every inflag / iceflag / liqflag branch of cldprop, including the 5-band (iceflag=1) cloud-band map."""
    d = make_gcm_inputs(128, 72, "cloudy", col0=77)
    d["inflglw"], d["iceflglw"], d["liqflglw"] = inflag, iceflag, liqflag
    if iceflag == 1:
        d["reice"] = np.asfortranarray(np.clip(d["reice"], 13.0, 130.0))
    if inflag == 0:
        tc = np.zeros((16, 128, 72), order="F")
        tc[:, :, 5:14] = np.linspace(0.1, 3.0, 16)[:, None, None] * d["cldfr"][None, :, 5:14]
        d["taucld"] = tc
    for icld in (1, 2):
        got = hip.rrtmg_lw_from_dict(d, icld=icld)
        ref = oracle.rrtmg_lw(128, 72, icld, 0, d)
        _compare(got, ref, 0, f"inflag{inflag} ice{iceflag} liq{liqflag} icld{icld}")


def test_prepared_column_entry(hip, oracle):
    """The post-inatm interface (the one the golden OUTPUT_RRTM files pin), total and per band."""
    import os
    from rrtmg_lw_amd.io_rrtm import read_input_rrtm
    g = os.path.join(os.path.dirname(__file__), "golden")
    col = read_input_rrtm(os.path.join(g, "input_rrtm_MLS-cld-imca0-icld2"), os.path.join(g, "in_cld_rrtm-cld5"))
    for istart, iend in [(1, 16), (3, 3), (16, 16)]:
        got = hip.run_columns([col, col], istart, iend)
        ref = oracle.column(col, istart, iend, iout=99 if istart > 1 else 0)
        for k in ("totuflux", "totdflux", "fnet", "htr", "totuclfl", "totdclfl", "fnetc", "htrc"):
            assert np.abs(got[k][0] - ref[k]).max() <= TIGHT_FLUX, (k, istart)
            assert np.array_equal(got[k][0], got[k][1])


@pytest.mark.parametrize("ncol,nlay", [(1, 72), (63, 51), (65, 72), (257, 33), (3, 4), (5, 200)])
def test_ragged_and_extreme_shapes(hip, oracle, ncol, nlay):
    """Single column, column counts that are not multiples of a wave / workgroup, four layers (the kissvec minimum) and
    more layers than any reference example (the reference's static arrays stop at mxlay = 203, parrrtm.f90)."""
    d = make_gcm_inputs(ncol, nlay, "cloudy" if nlay > 8 else "clear", col0=17)
    for icld in (1, 2):
        got = hip.rrtmg_lw_from_dict(d, icld=icld)
        ref = oracle.rrtmg_lw(ncol, nlay, icld, d["idrv"], d)
        _compare(got, ref, d["idrv"], f"ncol={ncol} nlay={nlay} icld={icld}")


def test_device_entry_with_caller_stream(hip, oracle):
    """Device-pointer entry: inputs and outputs are torch tensors in HBM, work is enqueued on the caller's stream and
    spans several internal batches (two-stream pipeline of the driver)."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    ncol, nlay = 1500, 72
    dev = torch.device("cuda", 0)
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=9, backend="torch", device=dev)
    outbuf = torch.full((output_rows(nlay), ncol), float("nan"), dtype=torch.float64, device=dev)
    out = output_views(outbuf, nlay)
    hip.set_batch(256)
    try:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hip.rrtmg_lw_device(d, out, stream=side.cuda_stream)
            hip.rrtmg_lw_device(d, out, stream=side.cuda_stream)        # back to back: prep sets are reused safely
        hip.check(side.cuda_stream)
    finally:
        hip.set_batch(0)
    dn = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=9)
    ref = oracle.rrtmg_lw(ncol, nlay, dn["icld"], dn["idrv"], dn)
    got = {k: out[k].T.cpu().numpy() for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")}
    got["icld"] = ref["icld"]
    _compare(got, ref, dn["idrv"], "device entry, 6 batches")


@pytest.mark.parametrize("config,ncol,nlay", [("cloudy", 1000, 72), ("clear", 3000, 40), ("aer_idrv", 700, 60)])
def test_small_calls_replayed_as_a_graph(hip, oracle, config, ncol, nlay):
    """A device-resident call of one batch is captured as a graph the second time it comes with the same arguments and replayed from then on
    (rrtmg_lw_hip_set_graph_max; driver.hip: run_pipelined): the outputs equal those of the plain launches bit for bit, a call with another
    output array gets a graph of its own, a larger call in between (the workspace grows: every graph is dropped) does no harm, and new
    input VALUES in the same arrays are what the replay computes with."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    dev = torch.device("cuda", 0)
    d = make_gcm_inputs(ncol, nlay, config, col0=77, backend="torch", device=dev)
    idrv = d["idrv"]
    stream = torch.cuda.current_stream().cuda_stream

    def run(n, buf):
        o = output_views(buf, nlay, idrv)
        for _ in range(n):
            hip.rrtmg_lw_device(d, o, stream=stream)
        hip.check(stream)
        return buf.clone()

    bufs = [torch.zeros((output_rows(nlay, idrv), ncol), dtype=torch.float64, device=dev) for _ in range(2)]
    prev = hip.set_graph_max(0)
    try:
        plain = run(2, bufs[0])
        hip.set_graph_max(1 << 20)
        c0, r0 = hip.graph_stats()
        got = run(5, bufs[0])                               # plain, captured, replayed x 3
        c1, r1 = hip.graph_stats()
        assert (c1 - c0, r1 - r0) == (1, 3)
        assert torch.equal(got.view(torch.int64), plain.view(torch.int64))
        got2 = run(3, bufs[1])                              # another output array: another key
        c2, r2 = hip.graph_stats()
        assert (c2 - c1, r2 - r1) == (1, 1)
        assert torch.equal(got2.view(torch.int64), plain.view(torch.int64))
        # new values in the same input arrays: the replay reads the arrays, not a copy
        tlay0 = d["tlay"].clone()
        d["tlay"] += 1.5
        warm = run(2, bufs[0])
        c3, r3 = hip.graph_stats()
        assert (c3 - c2, r3 - r2) == (0, 2)
        hip.set_graph_max(0)
        assert torch.equal(run(1, bufs[0]).view(torch.int64), warm.view(torch.int64))
        assert not torch.equal(warm, plain)
        d["tlay"].copy_(tlay0)
        # a larger call makes the workspace grow: the graphs go, the next small call starts over and still agrees
        hip.set_graph_max(1 << 20)
        big = make_gcm_inputs(4 * ncol + 333, nlay, config, col0=5, backend="torch", device=dev)
        bigbuf = torch.zeros((output_rows(nlay, idrv), 4 * ncol + 333), dtype=torch.float64, device=dev)
        hip.rrtmg_lw_device(big, output_views(bigbuf, nlay, idrv), stream=stream)
        hip.check(stream)
        again = run(4, bufs[0])
        assert torch.equal(again.view(torch.int64), plain.view(torch.int64))
    finally:
        hip.set_graph_max(prev)
    dn = make_gcm_inputs(ncol, nlay, config, col0=77)
    ref = oracle.rrtmg_lw(ncol, nlay, dn["icld"], idrv, dn)
    o = output_views(plain, nlay, idrv)
    gotd = {k: o[k].T.cpu().numpy() for k in o}
    gotd["icld"] = ref["icld"]
    _compare(gotd, ref, idrv, f"graph {config}")


def test_calls_from_several_threads(hip, oracle):
    """Concurrent callers get correct results (SURVEY.md 8b threading): calls of up to 8192 columns that arrive while another is in flight
    are solved together in one device pass (driver.hip: comb_call), larger ones and the other entries take turns at the entry lock."""
    import threading
    ds = [make_gcm_inputs(200, 40, "cloudy", col0=100 * k) for k in range(4)]
    res = [None] * 4

    def work(k):
        res[k] = hip.rrtmg_lw_from_dict(ds[k])

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(4):
        ref = oracle.rrtmg_lw(200, 40, ds[k]["icld"], ds[k]["idrv"], ds[k])
        _compare(res[k], ref, ds[k]["idrv"], f"thread {k}")


def test_reinitialisation(hip, oracle):
    """rrtmg_lw_ini may be called again (e.g. another cpdair): heating rates scale with 1/cpdair, fluxes do not change."""
    d = make_gcm_inputs(64, 40, "clear")
    a = hip.rrtmg_lw_from_dict(d)
    hip.rrtmg_lw_ini(1003.5, kdata=hip.STANDIN_KDATA, device=0)
    b = hip.rrtmg_lw_from_dict(d)
    hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    assert np.array_equal(a["uflx"], b["uflx"])
    np.testing.assert_allclose(b["hr"] * 1003.5, a["hr"] * 1004.0, rtol=1e-12, atol=1e-12)


def test_pinned_host_arrays_and_pipelined_batches(hip, oracle):
    """Host-pointer entry with arrays pinned through rrtmg_lw_hip_host_register and several column batches in flight
    (H2D | kernels | D2H pipeline): same results as with pageable arrays, and as the oracle."""
    d = make_gcm_inputs(1100, 51, "cloudy", col0=3)
    hip.set_batch(256)
    try:
        plain = hip.rrtmg_lw_from_dict(d)
        out = hip._out_arrays(1100, 51, d["idrv"])
        pinned = [v for v in list(d.values()) + list(out.values()) if isinstance(v, np.ndarray) and v.flags.f_contiguous and v.dtype == np.float64]
        for v in pinned:
            hip.host_register(v)
        got = hip.rrtmg_lw_from_dict(d, out=out)
        for v in pinned:
            hip.host_unregister(v)
    finally:
        hip.set_batch(0)
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
        assert np.array_equal(got[k], plain[k]), k
    ref = oracle.rrtmg_lw(1100, 51, d["icld"], d["idrv"], d)
    _compare(got, ref, d["idrv"], "pinned host arrays, 5 batches")


def _special_cloud_inputs(ncol, nlay, kind):
    """Cloud configurations the random synthetic set does not reach: prescribed cloud optical depths (inflag 0),
    overcast layers and equal fractions in adjacent layers (the `==` branches of rtrnmr's overlap factors)."""
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=55)
    rng = np.random.default_rng(7)
    cf = np.array(d["cldfr"])
    if kind == "inflag0":
        d["inflglw"], d["iceflglw"], d["liqflglw"] = 0, 0, 0
        tau = rng.uniform(0.05, 8.0, (16, ncol, nlay)) * (cf > 0)[None, :, :]
        d["taucld"] = np.asfortranarray(tau)
    elif kind == "overcast":
        cloudy = cf > 0
        cf[cloudy & (rng.random(cf.shape) < 0.4)] = 1.0
        for l in range(1, nlay):                      # equal fractions in neighbouring cloudy layers
            same = cloudy[:, l] & cloudy[:, l - 1] & (rng.random(ncol) < 0.3)
            cf[same, l] = cf[same, l - 1]
        d["cldfr"] = np.asfortranarray(cf)
    elif kind == "toplayer":                          # cloud in the top layer: nothing lies above the cloud zone (ltop = nlay)
        cf[:, nlay - 1] = np.where(rng.random(ncol) < 0.5, 0.6, 0.0)
        d["cldfr"] = np.asfortranarray(cf)
        for k in ("cliqwp", "cicewp"):
            a = np.array(d[k]); a[:, nlay - 1] = np.where(cf[:, nlay - 1] > 0, 20.0, 0.0); d[k] = np.asfortranarray(a)
    elif kind == "bottomonly":                        # clouds in the lowest layer only (ltop = 1)
        cf[:, 1:] = 0.0
        cf[:, 0] = np.where(rng.random(ncol) < 0.6, 0.7, 0.0)
        d["cldfr"] = np.asfortranarray(cf)
        for k in ("cliqwp", "cicewp"):
            a = np.array(d[k]); a[:, 1:] = 0.0; a[:, 0] = np.where(cf[:, 0] > 0, 30.0, 0.0); d[k] = np.asfortranarray(a)
    elif kind == "nocloud":                           # a cloudy-mode call whose batch holds no cloud at all (ltop = 0)
        d["cldfr"] = np.asfortranarray(cf * 0.0)
    elif kind == "thin":
        d["cldfr"] = np.asfortranarray(np.where(cf > 0, np.where(rng.random(cf.shape) < 0.5, 5e-7, 2e-6), 0.0))   # around rtrn's 1e-6 threshold
    return d


@pytest.mark.parametrize("kind", ["inflag0", "overcast", "thin", "toplayer", "bottomonly", "nocloud"])
@pytest.mark.parametrize("icld", [1, 2])
def test_special_cloud_configurations(hip, oracle, kind, icld, sweeps):
    ncol, nlay = 300, 60
    d = _special_cloud_inputs(ncol, nlay, kind)
    got = hip.rrtmg_lw_from_dict(d, icld=icld)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, d["idrv"], d)
    if kind == "toplayer":        # an (unphysical) water cloud in the 0.011 hPa thick top layer: own rate 5e4 K d-1
        _compare_thin_layers(got, ref, d, d["idrv"], f"{kind} icld={icld}")
    else:
        _compare(got, ref, d["idrv"], f"{kind} icld={icld}")
    if kind not in ("thin", "nocloud"):
        assert np.abs(ref["dflx"] - ref["dflxc"]).max() > 1.0


DIV_TOL = 2.5e-5     # W m-2: flux divergence of a layer (half of what two fluxes at TIGHT_FLUX each could differ by)
HEATFAC = 8.4391     # K d-1 per (W m-2 / hPa): g x 86400 / (cpdair x 100), src/rrtmg_lw_init.f90:298 with cpdair = 1004


def _compare_thin_layers(got, ref, d, idrv, tag):
    """Cloud decks that reach layers thinner than 1 hPa - down to 0.002 hPa: an unphysical stress of the sweeps' hand-off logic.  A heating
    rate IS the layer's flux divergence x 8.44 / dp[hPa] (src/rrtmg_lw_rtrn.f90:598), and an optically thick cloud in such a layer absorbs
    part of whatever error the upward flux carries INTO the layer from the column below (<= 1.4e-5 W m-2 = 3e-8 of the flux: the float32
    cell codes and table entries of every cell underneath; measured, profiles/round4_thin_layers.md: a float64 decode of the layer's own
    cells changes nothing) - x 460 at 0.018 hPa that is 5e-3 K d-1.  So the bars are: fluxes and d(flux)/dT as everywhere (5e-5); every
    layer's flux divergence within 2.5e-5 W m-2, i.e. every heating rate within max(5e-5 K d-1, 2.1e-4 / dp[hPa]) - the first term, the
    bar of every other test, decides for layers at least 4.2 hPa thick; and the north-star 1e-3 K d-1 in every layer at least 0.25 hPa thick."""
    dflux = max(np.abs(got[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    ddt = max(np.abs(got[k] - ref[k]).max() for k in ("duflx_dt", "duflxc_dt")) if idrv == 1 else 0.0
    dp = np.array(d["plev"])[:, :-1] - np.array(d["plev"])[:, 1:]
    err = np.stack([np.abs(got[k] - ref[k]) for k in ("hr", "hrc")])
    bound = np.maximum(TIGHT_HR, DIV_TOL * HEATFAC / dp)[None]
    worst = float((err / bound).max())
    i = np.unravel_index(err.argmax(), err.shape)
    thick = np.broadcast_to(dp[None] >= 0.25, err.shape)
    print(f"{tag}: max|dflux|={dflux:.3e} W/m2  max|d(dF/dT)|={ddt:.3e}  max|dhr|={err.max():.3e} K/d (layer {dp[i[1], i[2]]:.4f} hPa thick: "
          f"divergence error {err.max() * dp[i[1], i[2]] / HEATFAC:.2e} W/m2)  worst error / bound = {worst:.3f}  "
          f"max|dhr| in layers >= 0.25 hPa thick = {err[thick].max():.3e}")
    assert np.isfinite(got["uflx"]).all() and np.isfinite(got["hr"]).all()
    assert dflux <= TIGHT_FLUX and ddt <= TIGHT_FLUX
    assert worst <= 1.0 and err[thick].max() <= HR_TOL
    assert got["icld"] == ref["icld"]


def _block_top_inputs(ncol, nlay, tops, seed=5, bases=None):
    """Cloud decks whose top layer changes from one 64-column block to the next: block b reaches layer tops[b % len(tops)] (0 = the
    block holds no cloud), a third of its columns cloud-free, gaps inside the decks.  bases: the lowest cloudy layer of the block's
    decks (default 1), changing from block to block as well."""
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=17)
    rng = np.random.default_rng(seed)
    top = np.array([tops[(c // 64) % len(tops)] for c in range(ncol)])
    base = np.array([(bases[(c // 64) % len(bases)] if bases else 1) for c in range(ncol)])
    lay = np.arange(1, nlay + 1)[None, :]
    inside = (lay <= top[:, None]) & (lay >= base[:, None]) & (rng.random((ncol, 1)) < 0.67) & (rng.random((ncol, nlay)) < 0.8)
    # one column per cloudy block reaches the block's top for certain
    for b in range((ncol + 63) // 64):
        t = tops[b % len(tops)]
        if t > 0:
            inside[min(64 * b + 5, ncol - 1), t - 1] = True
            top[min(64 * b + 5, ncol - 1)] = t
    inside &= lay <= top[:, None]
    d["cldfr"] = np.asfortranarray(np.where(inside, 0.05 + 0.9 * rng.random((ncol, nlay)), 0.0))
    d["cliqwp"] = np.asfortranarray(np.where(inside, 60.0 * rng.random((ncol, nlay)), 0.0))
    d["cicewp"] = np.asfortranarray(np.where(inside, 20.0 * rng.random((ncol, nlay)), 0.0))
    d["reliq"] = np.asfortranarray(5.0 + 15.0 * rng.random((ncol, nlay)))
    d["reice"] = np.asfortranarray(15.0 + 85.0 * rng.random((ncol, nlay)))
    return d


@pytest.mark.parametrize("icld", [1, 2])
@pytest.mark.parametrize("idrv", [0, 1])
def test_cloud_top_changes_from_block_to_block(hip, oracle, icld, idrv, sweeps):
    """The sweeps hand over between the clear-sky kernels and the cloud-zone kernel at a level chosen per group of 64-column blocks
    (k_blocksort): neighbouring blocks with tops 0 / 14 / nlay / 1 / ..., more blocks than one hand-off group, a ragged last block."""
    nlay = 60
    ncol = 64 * 41 + 23
    d = _block_top_inputs(ncol, nlay, [0, 14, nlay, 1, 30, 0, 14, 59, 2, 45, 14, 14, 7])
    got = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, idrv, d)
    _compare_thin_layers(got, ref, d, idrv, f"block tops icld={icld} idrv={idrv}")
    assert np.abs(ref["dflx"] - ref["dflxc"]).max() > 1.0


@pytest.mark.parametrize("icld", [1, 2])
@pytest.mark.parametrize("idrv", [0, 1])
def test_cloud_base_changes_from_block_to_block(hip, oracle, icld, idrv, sweeps):
    """Below the lowest cloud of a group of blocks the cloud-zone sweep runs its clear-sky levels without the cloudy-level inputs
    (k_sweepz, layers 1 .. lbot - 1): decks with bases at layers 1 / 9 / 30 / top (one-layer decks) / nlay, next to blocks without cloud."""
    nlay = 60
    ncol = 64 * 29 + 11
    tops = [14, 20, 45, 30, 0, nlay, 12, 33, 9, 59, 25, 40, 16]
    bases = [1, 9, 30, 30, 1, nlay, 12, 2, 9, 50, 3, 39, 15]
    d = _block_top_inputs(ncol, nlay, tops, seed=13, bases=bases)
    got = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, idrv, d)
    _compare_thin_layers(got, ref, d, idrv, f"block bases icld={icld} idrv={idrv}")
    assert np.abs(ref["dflx"] - ref["dflxc"]).max() > 1.0


@pytest.mark.parametrize("config", ["cloudy_deep", "cloudy_towers", "cloudy_scatter", "cloudy_orography"])
def test_cloud_field_variants(hip, oracle, config, sweeps):
    ncol, nlay = 1500, 72
    d = make_gcm_inputs(ncol, nlay, config, col0=31 * 1000)
    got = hip.rrtmg_lw_from_dict(d)
    ref = oracle.rrtmg_lw(ncol, nlay, d["icld"], d["idrv"], d)
    _compare_thin_layers(got, ref, d, d["idrv"], config)      # (the towers reach layer 45 of 72: 2.5 hPa, 0.35 hPa thick)


def test_host_entry_skips_zero_rows_and_sums_taucld(hip, oracle):
    """The host-pointer entry does not copy (layer, band) rows of tauaer that are all zero for a column batch and, with inflglw >= 1,
    ships the band sum of taucld (cldprop's tauctot, src/rrtmg_lw_cldprop.f90:173-186) instead of taucld: isolated non-zero rows, a row
    that is non-zero in one batch only, -0.0 entries (not +0.0: copied), and the corner where the layer enters cldprop through
    tauctot alone (water path below cldmin = 1e-20, tauctot above / below it)."""
    ncol, nlay = 700, 40
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=3)
    rng = np.random.default_rng(8)
    ta = np.zeros((ncol, nlay, 16))
    ta[:, 3, 5] = 0.02 * rng.random(ncol)             # one isolated (layer, band) row
    ta[:, 10:13, :] = 0.01 * rng.random((ncol, 3, 16))  # a run of rows
    ta[300:, 20, 0] = 0.03                              # non-zero in the later batches only
    ta[5, 30, 7] = -0.0                                 # a negative zero is data
    ta[650, 39, 15] = 1e-300
    d["tauaer"] = np.asfortranarray(ta)
    # cloud layers that enter cldprop through tauctot only: tiny water paths, taucld summing to >= / < cldmin
    cf, ci, cl = (np.array(d[k]) for k in ("cldfr", "cicewp", "cliqwp"))
    tc = np.zeros((16, ncol, nlay))
    cf[::7, 20] = 0.4; ci[::7, 20] = 1e-25; cl[::7, 20] = 0.0
    tc[:, ::14, 20] = 1e-21                             # sum 1.6e-20 >= cldmin: enters (ncbands follows iceflag) ...
    tc[:, 7::14, 20] = 1e-22                            # ... sum 1.6e-21 < cldmin: does not
    d["cldfr"], d["cicewp"], d["cliqwp"], d["taucld"] = (np.asfortranarray(a) for a in (cf, ci, cl, tc))
    d["iceflglw"] = 1                                   # five cloud bands unless another layer sets sixteen
    hip.set_batch(256)
    try:
        for inflag in (2, 1, 0):
            d["inflglw"] = inflag
            if inflag == 0:
                tc0 = np.array(d["taucld"]); tc0[:, :, 5:9] = 0.3 * rng.random((16, ncol, 4)) * (cf[None, :, 5:9] > 0); d["taucld"] = np.asfortranarray(tc0)
            got = hip.rrtmg_lw_from_dict(d, icld=2)
            ref = oracle.rrtmg_lw(ncol, nlay, 2, d["idrv"], d)
            _compare(got, ref, d["idrv"], f"host entry, zero rows, inflag {inflag}")
    finally:
        hip.set_batch(0)


def test_host_entry_rows_that_do_not_travel(hip, oracle):
    """The host-pointer entry scans every row of every input array per column batch: a row holding ONE 8-byte pattern is filled on
    the device (k_fill_rows) instead of copied, the other rows are packed into pinned staging by host threads (pageable arrays) or
    leave from where they lie (pinned arrays).  Bit-equality of the three routes - device-resident inputs, pageable host arrays,
    pinned host arrays - on inputs with: well-mixed gases as constants, a gas row that is uniform in the first batch only, a row
    that differs in its LAST column only, a uniform row of -0.0 and one of a NaN-free denormal, uniform and non-uniform rows
    alternating (many short copy runs), a short last batch."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    ncol, nlay = 1000, 44
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=21)
    rng = np.random.default_rng(12)
    for k, v in (("co2vmr", 4.1e-4), ("ch4vmr", 1.8e-6), ("n2ovmr", 3.2e-7), ("o2vmr", 0.209), ("cfc11vmr", 2.3e-10), ("cfc22vmr", 0.0)):
        d[k] = np.asfortranarray(np.full((ncol, nlay), v))
    h2o = np.array(d["h2ovmr"]); h2o[:256, 30] = h2o[0, 30]; h2o[:, 31] = h2o[0, 31]; h2o[ncol - 1, 31] *= 1.01
    o3 = np.array(d["o3vmr"]); o3[:, ::2] = o3[0:1, ::2]                  # every other layer uniform
    d["h2ovmr"], d["o3vmr"] = np.asfortranarray(h2o), np.asfortranarray(o3)
    ta = np.array(d["tauaer"]); ta[:, 5, 3] = -0.0; ta[:, 6, 3] = 5e-324; ta[:, 7, :] = 0.013; ta[700:, 8, 2] = 0.02 * rng.random(300)
    d["tauaer"] = np.asfortranarray(ta)
    e = np.array(d["emis"]); e[:, 4] = 0.97
    d["emis"] = np.asfortranarray(e)
    dev = torch.device("cuda", 0)
    # device-resident copies with the Fortran arrays' memory order (the transpose of an F-ordered array is a C-ordered view of the same bytes)
    dd = {k: (torch.from_numpy(np.asfortranarray(v).T).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    hip.set_batch(256)
    try:
        plain = hip.rrtmg_lw_from_dict(d)
        out = hip._out_arrays(ncol, nlay, d["idrv"])
        pinned = [v for v in list(d.values()) + list(out.values()) if isinstance(v, np.ndarray) and v.flags.f_contiguous and v.dtype == np.float64]
        for v in pinned:
            hip.host_register(v)
        got = hip.rrtmg_lw_from_dict(d, out=out)
        for v in pinned:
            hip.host_unregister(v)
        outbuf = torch.full((output_rows(nlay), ncol), float("nan"), dtype=torch.float64, device=dev)
        oview = output_views(outbuf, nlay)
        hip.rrtmg_lw_device(dd, oview)
        hip.check()
    finally:
        hip.set_batch(0)
    names = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
    for k in names:
        assert np.array_equal(got[k], plain[k]), k
        assert np.array_equal(oview[k].T.cpu().numpy(), plain[k]), k
    ref = oracle.rrtmg_lw(ncol, nlay, d["icld"], d["idrv"], d)
    _compare(plain, ref, d["idrv"], "rows that do not travel")


def test_host_entry_ignores_cloud_arrays_where_no_column_has_cloud(hip, oracle):
    """A layer whose cloud fraction is below cldmin in every column of a batch: cldprop reads nothing else of it
    (src/rrtmg_lw_cldprop.f90:185-186), and the host-pointer entry does not read, sum, scan or copy the other cloud arrays there.
    Junk in those layers - water paths, optical depths, particle sizes outside the parameterisations' bounds, which would `stop` the
    reference in a cloudy layer - must change nothing; a layer that is cloud-free in some batches and cloudy in others; fractions of
    1e-21 (below cldmin) and of exactly cldmin."""
    ncol, nlay = 900, 40
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=5)
    rng = np.random.default_rng(4)
    cf = np.array(d["cldfr"])
    cf[:300, 20] = 0.0; cf[300:, 20] = np.where(rng.random(600) < 0.3, 0.5, 0.0)       # layer 21: cloud-free in the first batch only
    cf[:, 30] = 1e-21                                                                  # below cldmin everywhere
    cf[:, 31] = 0.0; cf[17, 31] = 1e-20                                                # one column exactly at cldmin
    free = (cf < 1e-20).all(axis=0)
    clean = {k: np.array(d[k]) for k in ("cicewp", "cliqwp", "reice", "reliq")}
    clean["cldfr"] = cf
    for k in ("cicewp", "cliqwp"):
        clean[k][:, 20] = np.where(cf[:, 20] > 0, 20.0, 0.0)
        clean[k][17, 31] = 5.0
    clean["reice"][:, 20] = 60.0; clean["reliq"][:, 20] = 10.0; clean["reice"][17, 31] = 60.0; clean["reliq"][17, 31] = 10.0
    tc = np.zeros((16, ncol, nlay))
    junk = {k: v.copy() for k, v in clean.items()}
    junk["cicewp"][:, free] = 1e3; junk["cliqwp"][:, free] = 7e2; junk["reice"][:, free] = 500.0; junk["reliq"][:, free] = 0.01
    junk["cicewp"][:300, 20] = 40.0; junk["reice"][:300, 20] = 1e4                       # (cloud-free for the first batch's columns only)
    tcj = tc.copy(); tcj[:, :, free] = 5.0; tcj[:, :300, 20] = 3.0
    hip.set_batch(300)
    try:
        for inflag in (2, 0):
            d["inflglw"] = inflag
            if inflag == 0:
                d["iceflglw"], d["liqflglw"] = 0, 0
                tc[:, :, 5:14] = 0.4 * (cf[None, :, 5:14] > 0); tcj[:, :, 5:14] = tc[:, :, 5:14]
            da = dict(d); da.update({k: np.asfortranarray(v) for k, v in clean.items()}); da["taucld"] = np.asfortranarray(tc)
            db = dict(d); db.update({k: np.asfortranarray(v) for k, v in junk.items()}); db["taucld"] = np.asfortranarray(tcj)
            a = hip.rrtmg_lw_from_dict(da, icld=2)
            b = hip.rrtmg_lw_from_dict(db, icld=2)
            for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
                assert np.array_equal(a[k], b[k]), (k, inflag)
            ref = oracle.rrtmg_lw(ncol, nlay, 2, d["idrv"], db)          # the oracle reads the junk the way the reference does: not at all
            _compare(b, ref, d["idrv"], f"junk in cloud-free layers, inflag {inflag}")
    finally:
        hip.set_batch(0)


def test_several_devices_from_one_process(hip, oracle):
    """rrtmg_lw_hip_init_devices: the host-pointer entries split their columns over the devices, one host thread each.  One GPU is
    reachable here, so the three devices are virtual ones on GPU 0 (separate workspaces, streams, table copies): results must equal
    the one-device call bit for bit (columns are independent), for a column count that is no multiple of 64, for one too small to
    split, with a physics error raised on a device other than the first, and for the McICA array entry."""
    from test_hip_mcica import _with_subcolumns
    ncol, nlay = 1000, 45
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=9)
    small = make_gcm_inputs(100, nlay, "cloudy", col0=2)
    dm = _with_subcolumns(oracle, make_gcm_inputs(400, nlay, "cloudy", col0=4), 2)
    one = hip.rrtmg_lw_from_dict(d, icld=2)
    one_small = hip.rrtmg_lw_from_dict(small)
    one_mc = hip.rrtmg_lw_mcica_from_dict(dm)
    try:
        hip.init_devices([0, 0, 0], kdata=hip.STANDIN_KDATA)
        assert hip.num_devices() == 3
        three = hip.rrtmg_lw_from_dict(d, icld=2)
        three_small = hip.rrtmg_lw_from_dict(small)
        three_mc = hip.rrtmg_lw_mcica_from_dict(dm)
        bad = dict(d)
        r = np.array(d["reice"]); r[900, 8] = 500.0          # a column of the third block
        bad["reice"] = np.asfortranarray(r)
        for k, v in (("cldfr", 0.5), ("cicewp", 10.0)):
            a = np.array(d[k]); a[900, 8] = v; bad[k] = np.asfortranarray(a)
        with pytest.raises(hip.RrtmgLwError, match="ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS"):
            hip.rrtmg_lw_from_dict(bad, icld=2)
        again = hip.rrtmg_lw_from_dict(d, icld=2)
    finally:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    assert hip.num_devices() == 1
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt"):
        assert np.array_equal(one[k], three[k]), k
        assert np.array_equal(one[k], again[k]), k
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
        assert np.array_equal(one_small[k], three_small[k]), k
        assert np.array_equal(one_mc[k], three_mc[k]), k
    _compare(three, oracle.rrtmg_lw(ncol, nlay, 2, 1, d), 1, "three virtual devices")


def test_device_entries_run_on_the_state_of_their_arrays(hip, oracle):
    """After rrtmg_lw_hip_init_devices the device-pointer entries pick the library state of the device their arrays live on
    (hipPointerGetAttributes).  One GPU is reachable here, so the three states are virtual devices on GPU 0, which take such calls in turn:
    three calls run on three different states (each with its own workspace, streams and tables) and give the one-device call's numbers bit
    for bit - non-McICA with d/dT over several batches, and the fused sub-column generator + McICA solver; a physics error raised on a
    state other than the first reaches rrtmg_lw_hip_check."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    dev = torch.device("cuda", 0)
    ncol, nlay = 900, 45
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=21, backend="torch", device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def solve(mc):
        buf = torch.zeros((output_rows(nlay, d["idrv"]), ncol), dtype=torch.float64, device=dev)
        o = output_views(buf, nlay, d["idrv"])
        if mc:
            hip.rrtmg_lw_mcica_subcol_device(d, o, 5, 0, icld=3, stream=stream)
        else:
            hip.rrtmg_lw_device(d, o, stream=stream)
        hip.check(stream)
        return buf.clone(), hip.last_device_state()

    one, st = solve(False)
    one_mc, _ = solve(True)
    assert st == 0
    prev_graph = hip.set_graph_max(0)
    try:
        hip.init_devices([0, 0, 0], kdata=hip.STANDIN_KDATA)
        hip.set_batch(256)
        seen = set()
        for _ in range(3):
            got, st = solve(False)
            seen.add(st)
            assert torch.equal(got.view(torch.int64), one.view(torch.int64))
        assert seen == {0, 1, 2}
        seen = set()
        for _ in range(3):
            got, st = solve(True)
            seen.add(st)
            assert torch.equal(got.view(torch.int64), one_mc.view(torch.int64))
        assert seen == {0, 1, 2}
        # an error on whichever state takes the call is found by check()
        bad = dict(d)
        r = d["reice"].clone(); r[800, 8] = 500.0
        bad["reice"] = r
        for k, v in (("cldfr", 0.5), ("cicewp", 10.0)):
            a = d[k].clone(); a[800, 8] = v; bad[k] = a
        for _ in range(2):
            buf = torch.zeros((output_rows(nlay, d["idrv"]), ncol), dtype=torch.float64, device=dev)
            hip.rrtmg_lw_device(bad, output_views(buf, nlay, d["idrv"]), stream=stream)
            with pytest.raises(hip.RrtmgLwError, match="ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS"):
                hip.check(stream)
        got, _ = solve(False)
        assert torch.equal(got.view(torch.int64), one.view(torch.int64))
    finally:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        hip.set_batch(0)
        hip.set_graph_max(prev_graph)
    dn = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=21)
    ref = oracle.rrtmg_lw(ncol, nlay, dn["icld"], dn["idrv"], dn)
    o = output_views(one, nlay, dn["idrv"])
    gotd = {k: o[k].T.cpu().numpy() for k in o}
    gotd["icld"] = ref["icld"]
    _compare(gotd, ref, dn["idrv"], "device entries by pointer")


@pytest.mark.parametrize("icld,idrv,ncol", [(2, 1, 70), (0, 0, 65), (1, 0, 64)])
def test_tallest_column_the_interface_accepts(hip, oracle, icld, idrv, ncol, sweeps):
    """nlay = 603 = mxlay of modules/parrrtm.f90:31, the largest value the entries accept: level tiles of k_flux, the sweeps' level loops,
    k_blocksort's histogram, 603 k_layer rows.  (Layers down to 0.002 hPa thick.)"""
    nlay = 603
    d = make_gcm_inputs(ncol, nlay, "aer_idrv" if idrv else "cloudy", col0=12)
    got = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, idrv, d)
    _compare_thin_layers(got, ref, d, idrv, f"603 layers icld={icld} idrv={idrv}")
    with pytest.raises(hip.RrtmgLwError, match="bad dimensions"):
        d604 = make_gcm_inputs(8, 604, "clear")
        hip.rrtmg_lw_from_dict(d604)


def test_device_entry_from_two_streams(hip, oracle):
    """Two callers enqueue device-resident work on different streams without synchronising in between: the driver orders the
    second call after the first (they share the workspace)."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    dev = torch.device("cuda", 0)
    ncol, nlay = 3000, 72
    da = make_gcm_inputs(ncol, nlay, "cloudy", col0=0, backend="torch", device=dev)
    db = make_gcm_inputs(ncol, nlay, "cloudy", col0=50_000, backend="torch", device=dev)
    oa = output_views(torch.zeros((output_rows(nlay), ncol), dtype=torch.float64, device=dev), nlay)
    ob = output_views(torch.zeros((output_rows(nlay), ncol), dtype=torch.float64, device=dev), nlay)
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    hip.set_batch(512)
    try:
        for _ in range(3):
            hip.rrtmg_lw_device(da, oa, stream=sa.cuda_stream)
            hip.rrtmg_lw_device(db, ob, stream=sb.cuda_stream)
        hip.check(sa.cuda_stream)
        hip.check(sb.cuda_stream)
    finally:
        hip.set_batch(0)
    for d0, o in ((0, oa), (50_000, ob)):
        dn = make_gcm_inputs(200, nlay, "cloudy", col0=d0)
        ref = oracle.rrtmg_lw(200, nlay, dn["icld"], dn["idrv"], dn)
        got = {k: o[k][:, :200].T.cpu().numpy() for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")}
        got["icld"] = ref["icld"]
        _compare(got, ref, 0, f"two streams, col0={d0}")


@pytest.mark.parametrize("config,mcica", [("cloudy", 0), ("aer_idrv", 0), ("cloudy", 5)])
def test_overlap_and_cu_partition_are_transparent(hip, config, mcica):
    """Device-pointer entries: k_layer of batch i + 1 beside the sweeps of batch i (rrtmg_lw_hip_set_overlap), and the two on their own
    compute units (rrtmg_lw_hip_set_cu_partition: streams with a CU mask; first / last batch on the whole chip) - several batches, the
    caller's stream the null stream and a stream of its own: the packed outputs equal the plain pipeline's bit for bit."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    dev = torch.device("cuda", 0)
    ncol, nlay = 5000, 40
    d = make_gcm_inputs(ncol, nlay, config, col0=77, backend="torch", device=dev)
    idrv = d["idrv"]
    alpha = None
    if mcica:
        dz = 29.2717 * d["tlay"] * torch.log(d["plev"][:, :-1] / d["plev"][:, 1:])
        a = torch.exp(-0.5 * (dz[:, 1:] + dz[:, :-1]) / 2500.0)
        alpha = torch.cat([torch.zeros_like(a[:, :1]), a], dim=1).t().contiguous().t()

    def run(stream):
        buf = torch.zeros((output_rows(nlay, idrv), ncol), dtype=torch.float64, device=dev)
        o = output_views(buf, nlay, idrv)
        if mcica:
            hip.rrtmg_lw_mcica_subcol_device(d, o, 1, 0, alpha=alpha, icld=mcica, stream=stream)
        else:
            hip.rrtmg_lw_device(d, o, stream=stream)
        hip.check(stream)
        return buf.cpu().numpy().view(np.int64)

    own = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    hip.set_batch(1024)
    try:
        plain = run(0)
        hip.set_overlap(True)
        over = run(0)
        hip.set_cu_partition(96)
        assert hip.cu_partition() == 96
        part0, part1 = run(0), run(own.cuda_stream)
        hip.set_cu_partition(200)                      # (rounded to the XCD count: 8 CUs per XCD left for the sweeps)
        assert hip.cu_partition() == 200
        part2 = run(own.cuda_stream)
    finally:
        hip.set_cu_partition(0)
        hip.set_overlap(False)
        hip.set_batch(0)
    assert hip.cu_partition() == 0
    for other in (over, part0, part1, part2):
        assert np.array_equal(plain, other)


@pytest.mark.parametrize("config,icld,idrv,mcica", [("cloudy", 2, 0, 0), ("cloudy_deep", 1, 1, 0), ("cloudy_towers", 2, 1, 0), ("cloudy", 2, 0, 5), ("cloudy_scatter", 2, 0, 2)])
def test_one_sweep_launch_is_transparent(hip, oracle, config, icld, idrv, mcica):
    """The cloud-zone kernel over all levels (small batches) against the three launches: the outputs are equal bit for bit - non-McICA
    rtrn / rtrnmr with and without d/dT, and the fused McICA entry (mask flavour of rtrnmc)."""
    ncol, nlay = 1700, 72
    d = make_gcm_inputs(ncol, nlay, config, col0=3)

    def run():
        if mcica:
            dz = np.full((ncol, nlay), 400.0)
            alpha = oracle.get_alpha(ncol, nlay, mcica, 0, 2500.0, dz, np.zeros(ncol), 100, d["cldfr"])
            return hip.rrtmg_lw_mcica_subcol_from_dict(d, 3, 0, icld=mcica, alpha=alpha, idrv=idrv)
        return hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)

    prev = hip.set_one_sweep_max(0)
    try:
        three = run()
        assert hip.set_one_sweep_max(1 << 30) == 0
        one = run()
    finally:
        hip.set_one_sweep_max(prev)
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if idrv else ()):
        assert np.array_equal(three[k], one[k]), k


@pytest.mark.parametrize("config,icld,idrv,mcica,one", [("cloudy", 2, 0, 0, True), ("cloudy_deep", 1, 1, 0, False), ("aer_idrv", 2, 1, 0, True),
                                                        ("clear", 0, 0, 0, False), ("clear", 0, 1, 0, False), ("cloudy", 2, 0, 5, True), ("cloudy_scatter", 2, 1, 2, False)])
def test_one_band_per_workgroup_is_transparent(hip, oracle, config, icld, idrv, mcica, one):
    """Batches too small to fill the chip are swept one band per workgroup, a flux partial per band (rrtmg_lw_hip_set_split_max); k_flux adds
    the bands of a group first, in the order the group's workgroup adds them in LDS otherwise: the outputs equal those of the grouped
    sweeps bit for bit - cloud-free, rtrn / rtrnmr with and without d/dT, the fused McICA entry; with the one sweep launch and with the
    three; a column count that ends inside a block; and batches of a call that are small enough next to the call's first, larger one."""
    ncol, nlay = 700 + 37, 72
    d = make_gcm_inputs(ncol, nlay, config, col0=3)

    def run():
        if mcica:
            dz = np.full((ncol, nlay), 400.0)
            alpha = oracle.get_alpha(ncol, nlay, mcica, 0, 2500.0, dz, np.zeros(ncol), 100, d["cldfr"])
            return hip.rrtmg_lw_mcica_subcol_from_dict(d, 3, 0, icld=mcica, alpha=alpha, idrv=idrv)
        return hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)

    prev_one = hip.set_one_sweep_max((1 << 30) if one else 0)
    prev = hip.set_split_max(0)
    try:
        grouped = run()
        assert hip.set_split_max(1 << 20) == 0
        split = run()
        hip.set_batch(512)                  # two batches: 512 columns, then 225
        split2 = run()
    finally:
        hip.set_batch(0)
        hip.set_split_max(prev)
        hip.set_one_sweep_max(prev_one)
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if idrv else ()):
        assert np.array_equal(grouped[k], split[k]), k
        assert np.array_equal(grouped[k], split2[k]), (k, "two batches")
    assert np.abs(grouped["uflx"]).max() > 100.0


@pytest.mark.parametrize("config,ncol,nlay,icld,idrv,mcica", [("cloudy", 300, 72, 2, 0, 0), ("cloudy", 1024, 72, 1, 1, 0), ("clear", 700, 51, 0, 0, 0),
                                                              ("cloudy_orography", 341, 72, 2, 0, 0), ("cloudy_orography", 117, 72, 3, 0, 0),
                                                              ("aer_idrv", 130, 137, 2, 1, 0), ("cloudy", 200, 72, 2, 0, 5), ("cloudy", 1900, 40, 2, 0, 0)])
def test_bands_over_several_workgroups_are_transparent(hip, oracle, config, ncol, nlay, icld, idrv, mcica):
    """A batch whose (window, layer) pairs do not fill the chip spreads k_layer's sixteen bands of a pair over two or four workgroups along the
    staging passes (rrtmg_lw_hip_set_layer_split; both launches, narrow and wide - the terrain cases): same cells, same arithmetic, the
    outputs bit for bit those of one workgroup per pair - rtrn / rtrnmr / clear, d/dT, 137 layers, the fused McICA entry, a layer count that
    gives two parts instead of four; and against the oracle."""
    d = make_gcm_inputs(ncol, nlay, config, col0={341: 282237, 117: 844914}.get(ncol, 9))

    def run():
        if mcica:
            dz = np.full((ncol, nlay), 400.0)
            alpha = oracle.get_alpha(ncol, nlay, mcica, 0, 2500.0, dz, np.zeros(ncol), 100, d["cldfr"])
            return hip.rrtmg_lw_mcica_subcol_from_dict(d, 3, 0, icld=mcica, alpha=alpha, idrv=idrv)
        return hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)

    prev = hip.set_layer_split(0)
    try:
        one = run()
        assert hip.set_layer_split(1) == 0
        parts = run()
    finally:
        hip.set_layer_split(prev)
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if idrv else ()):
        assert np.array_equal(one[k], parts[k]), k
    if not mcica:
        _compare(parts, oracle.rrtmg_lw(ncol, nlay, icld, idrv, d), idrv, f"bands over several workgroups {config} {ncol}x{nlay}")


def test_band_ranges_with_bands_over_several_workgroups(hip, oracle):
    """The prepared-column entry with a band range (istart .. iend) on a batch small enough for the split: a workgroup takes the bands of its
    part that lie in the range."""
    import os
    from rrtmg_lw_amd.io_rrtm import read_input_rrtm
    G = os.path.join(os.path.dirname(__file__), "golden")
    col = read_input_rrtm(os.path.join(G, "input_rrtm_MLS-cld-imca0-icld2"), os.path.join(G, "in_cld_rrtm-cld5"))
    for a, b in ((1, 16), (1, 7), (5, 5), (16, 16), (1, 12)):
        outs = []
        for on in (0, 1):
            prev = hip.set_layer_split(on)
            try:
                outs.append(hip.run_columns([col] * 70, a, b, icld=2))
            finally:
                hip.set_layer_split(prev)
        for k in ("totuflux", "totdflux", "htr"):
            assert np.array_equal(outs[0][k], outs[1][k]), (a, b, k)
        ref = oracle.column(col, a, b, 99 if a == b else 0, icld=2)
        assert np.abs(outs[1]["totuflux"] - ref["totuflux"][None, :]).max() <= 5e-5, (a, b)


@pytest.mark.parametrize("config,icld,idrv", [("cloudy_scatter", 2, 0), ("cloudy_deep", 2, 0), ("cloudy_deep", 1, 0), ("aer_idrv", 2, 1), ("cloudy", 2, 0)])
def test_column_order_is_transparent(hip, oracle, config, icld, idrv):
    """k_colsort takes the columns of a cloudy batch by cloud top within windows of 256 where that pays (rrtmg_lw_hip_set_column_sort): the
    caller's arrays are read and written through that order and the outputs are equal bit for bit to those of the columns as they lie -
    every window reordered (threshold 0), the default threshold, a column count that ends inside a window, several batches per call, and
    against the oracle."""
    ncol, nlay = 1333, 72
    d = make_gcm_inputs(ncol, nlay, config, col0=40)
    prev_min = hip.column_sort_min()
    prev = hip.set_column_sort(False)
    prev_one = hip.set_one_sweep_max(0)         # (a batch this small would otherwise take the one sweep launch, for which no order is made)
    try:
        plain = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
        res = {}
        for name, mn, batch in (("every window", 0, 131072), ("default threshold", 24, 131072), ("three batches", 0, 512)):
            hip.set_column_sort(True, mn)
            hip.set_batch(batch)
            res[name] = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
    finally:
        hip.set_batch(0)
        hip.set_column_sort(prev, prev_min)
        hip.set_one_sweep_max(prev_one)
    for name, got in res.items():
        for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if idrv else ()):
            assert np.array_equal(plain[k], got[k]), (name, k)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, idrv, d)
    _compare_thin_layers(res["every window"], ref, d, idrv, f"column order {config} icld={icld}")


def test_workspace_grows_with_call_shapes(hip, oracle):
    """The per-batch workspace holds what the call shapes seen so far need (partial slabs of 4 band groups without d/dT and up to 8 with,
    the d/dT slab, rtrn's emissivity term, rtrnmr's overlap factors): a library initialised afresh sees the shapes in an order that makes
    it grow at every step, then in reverse, and every result equals the one a fresh library gives for that shape alone."""
    ncol, nlay = 900, 50
    shapes = [("clear", 0, 0), ("cloudy", 2, 0), ("cloudy", 1, 0), ("aer_idrv", 2, 1), ("aer_idrv", 1, 1)]
    inputs = {sh: make_gcm_inputs(ncol, nlay, sh[0], col0=70) for sh in shapes}
    alone = {}
    for sh in shapes:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        alone[sh] = hip.rrtmg_lw_from_dict(inputs[sh], icld=sh[1], idrv=sh[2])
    hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    sizes = []
    for sh in shapes + shapes[::-1]:
        got = hip.rrtmg_lw_from_dict(inputs[sh], icld=sh[1], idrv=sh[2])
        sizes.append(hip.workspace_bytes())
        for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if sh[2] else ()):
            assert np.array_equal(got[k], alone[sh][k]), (sh, k)
    assert sizes[0] < sizes[1] <= sizes[2] < sizes[3] and sizes[4] == sizes[-1], sizes
    ref = oracle.rrtmg_lw(ncol, nlay, 1, 1, inputs[shapes[-1]])
    _compare(alone[shapes[-1]], ref, 1, "rtrn + aerosol + d/dT on a fresh workspace")


def test_static_arrays_are_scanned_once(hip, oracle):
    """rrtmg_lw_hip_host_static: the row scans of a declared array are kept per column batch; rrtmg_lw_hip_host_changed drops them.  Same
    numbers with and without the declaration, over several batches; a change announced by host_changed is seen, rows of a static array
    that are not uniform still travel (a gas profile that varies from column to column), and withdrawing the declaration works."""
    ncol, nlay = 2500, 40
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=21)
    hip.set_batch(1024)
    try:
        want = hip.rrtmg_lw_from_dict(d, icld=2)
        static = [d[k] for k in ("tauaer", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "emis", "o3vmr")]     # (o3vmr varies per column: non-uniform rows)
        for a in static:
            hip.host_static(a)
        first = hip.rrtmg_lw_from_dict(d, icld=2)
        second = hip.rrtmg_lw_from_dict(d, icld=2)                # every declared row comes from the cache
        co2 = d["co2vmr"]
        co2 *= 2.0                                                # the host model changes a static array ...
        hip.host_changed(co2)                                     # ... and says so
        changed = hip.rrtmg_lw_from_dict(d, icld=2)
        ref = oracle.rrtmg_lw(ncol, nlay, 2, d["idrv"], d)
        aer = d["tauaer"]
        aer[:, :5, :] *= 0.5
        hip.host_changed(aer, keep=False)                         # declaration withdrawn: scanned on every call again
        undeclared = hip.rrtmg_lw_from_dict(d, icld=2)
        ref2 = oracle.rrtmg_lw(ncol, nlay, 2, d["idrv"], d)
        with pytest.raises(hip.RrtmgLwError, match="no static range"):
            hip.host_changed(aer)
    finally:
        for a in static:
            try:
                hip.host_changed(a, keep=False)
            except hip.RrtmgLwError:
                pass
        hip.set_batch(0)
    for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt"):
        assert np.array_equal(want[k], first[k]) and np.array_equal(want[k], second[k]), k
    assert np.abs(changed["uflx"] - want["uflx"]).max() > 0.1
    _compare(changed, ref, 1, "static co2vmr doubled, host_changed")
    _compare(undeclared, ref2, 1, "tauaer halved after its declaration was withdrawn")


def test_concurrent_callers_are_combined(hip, oracle):
    """Several threads call the host-pointer entry at once with chunks of a few columns (an OpenMP host model): calls that arrive while
    another is in flight are solved together in one device pass (driver.hip, comb_call).  Every chunk's result equals that of the same
    columns in one big call bit for bit, a chunk with a physics error fails alone and its caller reads ITS error text; and calls that wait
    while another holds the turn are served in fewer passes than there are calls."""
    import threading
    ncol, nlay, chunk, nthreads = 1536, 40, 32, 8
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=64)
    whole = hip.rrtmg_lw_from_dict(d)
    keys = [k for k, v in d.items() if isinstance(v, np.ndarray)]

    def part(c0, c1):
        p = dict(d)
        p["ncol"] = c1 - c0
        for k in keys:
            v = d[k]
            if v.ndim == 1:
                p[k] = np.ascontiguousarray(v[c0:c1])
            elif k == "taucld":
                p[k] = np.asfortranarray(v[:, c0:c1, :])
            else:
                p[k] = np.asfortranarray(v[c0:c1])
        return p

    chunks = [part(c0, min(ncol, c0 + chunk)) for c0 in range(0, ncol, chunk)]
    bad = 17
    r = np.array(chunks[bad]["reice"]); r[3, 8] = 500.0
    chunks[bad]["reice"] = np.asfortranarray(r)
    for k, v in (("cldfr", 0.5), ("cicewp", 10.0)):
        a = np.array(chunks[bad][k]); a[3, 8] = v; chunks[bad][k] = np.asfortranarray(a)
    bad2 = 30                                                     # a second caller's error, another text: each thread reads its own
    r = np.array(chunks[bad2]["reliq"]); r[5, 9] = 1.0
    chunks[bad2]["reliq"] = np.asfortranarray(r)
    for k, v in (("cldfr", 0.5), ("cliqwp", 10.0)):
        a = np.array(chunks[bad2][k]); a[5, 9] = v; chunks[bad2][k] = np.asfortranarray(a)
    results, errors = [None] * len(chunks), [None] * len(chunks)
    calls0, passes0 = hip.combine_stats()

    def worker(t):
        for rep in range(2):                                      # (the second round finds the others in flight for certain)
            for i in range(t, len(chunks), nthreads):
                try:
                    results[i] = hip.rrtmg_lw_from_dict(chunks[i])
                except hip.RrtmgLwError as e:
                    errors[i] = str(e)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    calls, passes = hip.combine_stats()
    print(f"combining entry: {calls - calls0} calls in {passes - passes0} device passes")
    assert calls - calls0 == 2 * len(chunks)
    # That calls ARE combined is shown apart from the bad chunks (a group that holds a physics error costs 1 + n passes for its n calls)
    # and without leaning on how eight Python threads happen to interleave: one call of a few thousand columns holds the turn while
    # twelve small ones arrive; whoever takes the turn next serves all that wait in ONE pass.  (A loaded machine may start the small
    # calls late: three attempts.)
    big = part(0, ncol)
    small = [c for i, c in enumerate(chunks[:14]) if i not in (bad, bad2)][:12]
    combined = False
    for attempt in range(3):
        c0_, p0_ = hip.combine_stats()
        started = threading.Event()

        def lead():
            started.set()
            hip.rrtmg_lw_from_dict(big)

        def follow(c):
            started.wait()
            hip.rrtmg_lw_from_dict(c)

        th = [threading.Thread(target=lead)] + [threading.Thread(target=follow, args=(c,)) for c in small]
        for x in th:
            x.start()
        for x in th:
            x.join()
        c1_, p1_ = hip.combine_stats()
        print(f"  one call of {ncol} columns + {len(small)} calls of {chunk}: {c1_ - c0_} calls in {p1_ - p0_} passes")
        assert c1_ - c0_ == 1 + len(small)
        if p1_ - p0_ < c1_ - c0_:
            combined = True
            break
    assert combined
    for i, c0 in enumerate(range(0, ncol, chunk)):
        if i == bad:
            assert errors[i] and "ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS" in errors[i]
            continue
        if i == bad2:
            assert errors[i] and "LIQUID EFFECTIVE RADIUS OUT OF BOUNDS" in errors[i]
            continue
        assert errors[i] is None, (i, errors[i])
        for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"):
            assert np.array_equal(results[i][k], whole[k][c0:c0 + chunk]), (i, k)


@pytest.mark.parametrize("icld,lo", [(2, 0.45), (0, 0.70)])
def test_orography_spread_of_pressure_levels(hip, oracle, icld, lo):
    """Neighbouring columns on very different pressure grids (surface pressure 45 % ... 105 % of 1013 hPa, as over steep
    orography with terrain-following levels): within one k_layer workgroup the reference-pressure index jp then spans several
    values and tropospheric and stratospheric cells share a layer index, so cells fall outside the absorption-table window staged
    in LDS and whole waves take the global-memory evaluation instead.  Both evaluations must give the oracle's numbers."""
    ncol, nlay = 700, 72
    d = make_gcm_inputs(ncol, nlay, "cloudy", col0=4242)
    rng = np.random.default_rng(11)
    f = rng.uniform(lo, 1.05, ncol)
    f[::7] = 1.0                                           # a few standard columns in between
    for k in ("play", "plev"):
        d[k] = np.asfortranarray(np.array(d[k]) * f[:, None])
    got = hip.rrtmg_lw_from_dict(d, icld=icld)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, d["idrv"], d)
    _compare(got, ref, d["idrv"], f"orography icld={icld}")
    jp = np.floor(36.0 - 5.0 * (np.log(np.array(d["play"])) + 0.04)).astype(int)
    assert (jp.max(axis=0) - jp.min(axis=0)).max() >= 3        # the spread the staging window cannot hold


@pytest.mark.parametrize("col0,ncol", [(844914, 117), (282237, 341), (903511, 237), (662926, 103), (959099, 417)])
def test_last_window_with_a_cloudy_last_column(hip, oracle, col0, ncol):
    """Regression (round 5, profiles/round5_exec_hazard.md): a ragged last window whose LAST column is cloudy in some layer.  k_layer's
    threads past the last column shadow it; compiled without -mllvm -amdgpu-remove-redundant-endcf=0 their registers were left
    clobbered behind the cloudy branch (copies of the register allocator ran under the `if (incol)` mask), the next staging pass copied
    rows from wrong places, and whole waves of the window came out with band 5's optical depths wrong (up to 0.6 W m-2).  The five calls
    are the ones a random sweep over terrain-following grids found; each must agree with the narrow-window run bit for bit, in every
    cloud mode, and with the oracle."""
    nlay = 72
    d = make_gcm_inputs(ncol, nlay, "cloudy_orography", col0=col0)
    assert (np.array(d["cldfr"])[-1] > 0).any()
    for icld in (1, 2, 3):
        outs = {}
        for on in (1, 0):
            prev = hip.set_wide_window(on)
            try:
                outs[on] = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=0)
            finally:
                hip.set_wide_window(prev)
        for k in outs[1]:
            assert np.array_equal(outs[1][k], outs[0][k]), (k, icld)
        _compare(outs[1], oracle.rrtmg_lw(ncol, nlay, icld, 0, d), 0, f"ragged cloudy last window icld={icld}")
    outs = {}
    for on in (1, 0):       # the mask flavour of the McICA kernels (k_layer<mcmask>)
        prev = hip.set_wide_window(on)
        try:
            outs[on] = hip.rrtmg_lw_mcica_subcol_from_dict(d, 7, 0, icld=2, idrv=0)
        finally:
            hip.set_wide_window(prev)
    for k in outs[1]:
        assert np.array_equal(outs[1][k], outs[0][k]), (k, "mcica")


@pytest.mark.parametrize("icld,idrv,mcica", [(0, 0, 0), (2, 1, 0), (1, 0, 0), (2, 0, 2)])
def test_wide_window_is_transparent(hip, oracle, icld, idrv, mcica):
    """k_layer takes a workgroup whose 256 columns lie more than one reference-pressure plane apart (a terrain-following grid: synth
    "cloudy_orography") in a second launch that stages five planes of the absorption tables instead of three
    (rrtmg_lw_hip_set_wide_window).  The same table entries either way: the fluxes with the second launch, without it (every workgroup on
    the narrow window, the cells outside it through global memory) and of a flat grid's call (no workgroup on the list) agree bit for
    bit with what they were, several batches and a ragged last window included; and the list is empty again for the next call."""
    ncol, nlay = 2 * 256 + 77, 72
    d = make_gcm_inputs(ncol, nlay, "cloudy_orography", col0=9000)
    jp = np.floor(36.0 - 5.0 * (np.log(np.array(d["play"])) + 0.04)).astype(int)
    assert (jp.max(axis=0) - jp.min(axis=0)).max() >= 2        # the spread the narrow window cannot hold
    outs = {}
    hip.set_batch(256)
    try:
        for on in (1, 0, 1):
            prev = hip.set_wide_window(on)
            try:
                if mcica:       # the fused generator + McICA solver entry (k_layer<mcmask>)
                    got = hip.rrtmg_lw_mcica_subcol_from_dict(d, 7, 0, icld=mcica, idrv=idrv)
                    if on in outs:
                        for k in got:
                            assert np.array_equal(got[k], outs[on][k]), (k, "second call with the wide window")
                    outs[on] = got
                else:
                    got = hip.rrtmg_lw_from_dict(d, icld=icld, idrv=idrv)
                    if on in outs:
                        for k in got:
                            assert np.array_equal(got[k], outs[on][k]), (k, "second call with the wide window")
                    outs[on] = got
            finally:
                hip.set_wide_window(prev)
    finally:
        hip.set_batch(0)
    for k in outs[1]:
        assert np.array_equal(outs[1][k], outs[0][k]), k
    if not mcica:
        ref = oracle.rrtmg_lw(ncol, nlay, icld, idrv, d)
        _compare(outs[1], ref, idrv, f"wide window icld={icld} idrv={idrv}")
        flat = make_gcm_inputs(ncol, nlay, "cloudy", col0=9000)         # a call without a single workgroup on the list, after one with
        _compare(hip.rrtmg_lw_from_dict(flat, icld=icld, idrv=idrv), oracle.rrtmg_lw(ncol, nlay, icld, idrv, flat), idrv, "flat grid after orography")


def test_chunk_queue_equals_one_call(hip, oracle):
    """A host model that hands over ragged chunks of a few dozen columns (rrtmg_lw_hip_queue_*): one aggregated pass gives every chunk
    exactly what a single call over all columns gives, for rtrnmr with aerosol and dF/dT and for a cloud-free call."""
    for config, icld in (("aer_idrv", 2), ("cloudy", 0)):
        ncol, nlay = 333, 40
        d = make_gcm_inputs(ncol, nlay, config, col0=123)
        whole = hip.rrtmg_lw_from_dict(d, icld=icld)
        q = hip.ChunkQueue(nlay, icld, d["idrv"], d["inflglw"], d["iceflglw"], d["liqflglw"])
        bounds = [0, 1, 17, 64, 65, 200, 333]
        outs = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            c = {k: (np.asfortranarray(v[:, a:b, :]) if k == "taucld" else np.asfortranarray(v[a:b])) if isinstance(v, np.ndarray) else v
                 for k, v in d.items()}
            c["ncol"] = b - a
            outs.append(q.add(c))
        assert q.columns() == ncol
        q.flush()
        assert q.columns() == 0
        keys = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if d["idrv"] else ())
        for (a, b), o in zip(zip(bounds[:-1], bounds[1:]), outs):
            for k in keys:
                assert np.array_equal(o[k], whole[k][a:b]), (config, a, k)
    ref = oracle.rrtmg_lw(ncol, nlay, 0, 0, d)
    assert np.abs(whole["uflx"] - ref["uflx"]).max() <= TIGHT_FLUX


def test_north_star_mapping_prototype(hip, oracle):
    """k_n1 (rrtmg_lw_hip_set_n1_prototype): one column per wavefront, g-points across lanes, wave-reduce over all bands, final fluxes
    and heating rates written by the sweep itself ("north-star mapping").  Kept as a measured prototype for cloud-free calls;
    it must give the oracle's numbers.  The switch is an explicit call (an environment variable must not pick the numerical path)."""
    d = make_gcm_inputs(130, 72, "clear", col0=7)
    da = make_gcm_inputs(70, 51, "aer_idrv", col0=3)
    assert hip.lib().rrtmg_lw_hip_n1_prototype() == 0
    hip.set_n1_prototype(True)
    try:
        assert hip.lib().rrtmg_lw_hip_n1_prototype() == 1
        got = hip.rrtmg_lw_from_dict(d, icld=0)
        gota = hip.rrtmg_lw_from_dict(da, icld=0, idrv=0)           # aerosol, perturbed columns
    finally:
        hip.set_n1_prototype(False)
    _compare(got, oracle.rrtmg_lw(130, 72, 0, 0, d), 0, "k_n1 clear 72")
    _compare(gota, oracle.rrtmg_lw(70, 51, 0, 0, da), 0, "k_n1 aerosol 51")
    again = hip.rrtmg_lw_from_dict(d, icld=0)                        # the production path, after the switch is off again
    assert np.abs(again["uflx"] - got["uflx"]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("config,nlay,icld,ncol", [("cloudy", 72, 2, 24576), ("aer_idrv", 137, 2, 6144), ("clear", 72, 0, 16384)])
def test_large_sample_parity(hip, oracle, config, nlay, icld, ncol):
    """Tens of thousands of columns (3.4 million cells x 140 g-points in the first case) against the oracle: the per-cell decisions -
    series or table, the table index formed with the reciprocal-based division - are the only place where a last-bit difference could
    show as more than rounding, one table step (~1e-6 W m-2 per cell) at a time; the worst column must stay inside the regression bar,
    and the sample spans more than one device batch boundary when the batch is set small."""
    d = make_gcm_inputs(ncol, nlay, config, col0=100000)
    hip.set_batch(8192)
    try:
        got = hip.rrtmg_lw_from_dict(d, icld=icld)
    finally:
        hip.set_batch(0)
    ref = oracle.rrtmg_lw(ncol, nlay, icld, d["idrv"], d)
    dflux = max(np.abs(got[k] - ref[k]).max() for k in ("uflx", "dflx", "uflxc", "dflxc"))
    dhr = max(np.abs(got[k] - ref[k]).max() for k in ("hr", "hrc"))
    print(f"large sample {config} L{nlay} icld{icld} x {ncol}: max|dflux|={dflux:.3e} max|dhr|={dhr:.3e}")
    assert dflux <= 0.01 and dhr <= 0.001
    assert dflux <= 5e-5 and dhr <= 5e-5
    if d["idrv"]:
        assert max(np.abs(got[k] - ref[k]).max() for k in ("duflx_dt", "duflxc_dt")) <= 5e-5
