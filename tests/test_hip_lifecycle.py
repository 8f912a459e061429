"""State that outlives a call: what the driver keeps between calls - the tables of the last initialisation, the graphs of small
device-resident calls, the workspace and its row stride, the batch size, the tuning switches - and what it must NOT keep.  The other GPU
tests compute one call in a freshly prepared library and compare it with the oracle; the subject here is the SEQUENCE of calls:

 * a re-initialisation (another cpdair, other absorption coefficients) under a live graph: the graph's kernel nodes hold the tables by
   value, and the allocations of the new initialisation usually come back at the addresses of the old one;
 * a seeded sequence of some forty operations (re-initialisations, device sets, the other g-point model, batch sizes, workspace growth,
   tuning switches, failing calls) after each of which a fixed set of probe calls must give the bits it gave in a fresh library;
 * a batch whose workspace rows lie more than 2^31 bytes behind the start of their array: the sweeps read rows through a buffer descriptor
   of 0x7ffffff0 bytes with the row as a scalar byte offset (kernels.hip: sweep_rsrc, bload_*'s soff);
 * the batch size in force (rrtmg_lw_hip_effective_batch): its defaults, and that it keeps those rows inside the descriptor;
 * three cycles of rrtmg_lw_ini .. finalize in one process with a call per family of GPU resources the driver owns (driver.hip, "who
   owns what"), and a process that ends without finalize: nothing of the library runs at exit.

Every test leaves the library as the session fixture made it: 140 g-points, stand-in k-data, cpdair 1004.0, device 0, set_batch(0), every
switch at its previous value."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rrtmg_lw_amd.blob import read_blob, write_blob
from rrtmg_lw_amd.synth import make_gcm_inputs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_parity import _compare, _compare_thin_layers  # noqa: E402
from test_hip_spectral import _check_sums, _nan_out, inatm  # noqa: E402

gpu = pytest.mark.gpu

STANDIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rrtmg_lw_amd", "data", "standin.kdata.bin")
OUT6 = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
SWEEP_RANGE = 0x7ffffff0        # num_records of the sweeps' buffer descriptors (kernels.hip: sweep_rsrc)


def _as_session(hip):
    """the library as the session fixture made it"""
    hip.select_gpoints(140)
    hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    hip.set_batch(0)


def _bits(t):
    import torch
    return t.view(torch.int64)


class _DeviceCall:
    """One device-resident call of one batch with ITS arrays: the same input tensors and the same output buffer every time, which is what
    makes the driver capture it as a graph the second time and replay it from then on (driver.hip: run_pipelined)."""

    def __init__(self, hip, ncol, nlay, config, idrv, col0=77):
        import torch
        from rrtmg_lw_amd.shard import output_rows, output_views
        self.hip, self.torch, self.ncol, self.nlay, self.idrv = hip, torch, ncol, nlay, idrv
        dev = torch.device("cuda", 0)
        self.d = make_gcm_inputs(ncol, nlay, config, col0=col0, backend="torch", device=dev)
        self.buf = torch.zeros((output_rows(nlay, idrv), ncol), dtype=torch.float64, device=dev)
        self.out = output_views(self.buf, nlay, idrv)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.host = make_gcm_inputs(ncol, nlay, config, col0=col0)

    def run(self, n=1):
        self.buf.fill_(float("nan"))
        for _ in range(n):
            self.hip.rrtmg_lw_device(self.d, self.out, icld=2, idrv=self.idrv, stream=self.stream)
        self.hip.check(self.stream)
        return self.buf.clone()

    def named(self, buf):
        from rrtmg_lw_amd.shard import output_views
        o = output_views(buf, self.nlay, self.idrv)
        return {k: o[k].T.cpu().numpy() for k in o}


def _capture(hip, call):
    """plain launches, capture, replay: afterwards the call's graph is live"""
    c0, r0 = hip.graph_stats()
    got = call.run(3)
    c1, r1 = hip.graph_stats()
    assert c1 - c0 == 1 and r1 - r0 >= 1, (c1 - c0, r1 - r0)
    return got


# -------------------------------------------------------------------------------------------- 1a. re-init under a live graph: cpdair
@gpu
def test_reinit_with_another_cpdair_under_a_live_graph(hip, oracle):
    """rrtmg_lw_ini(another cpdair) while the graph of a small device-resident call is live, the call's tensors untouched: every call after
    it equals the plain launches of the new initialisation bit for bit - fluxes as before, heating rates x 1004.0 / 1003.5 (the bar of
    test_reinitialisation) - and the first of them is not a replay: a re-initialisation drops the graphs whatever addresses its
    allocations come back with (captures, replays over the three calls that follow: 1, 1).

    Before the fix init_state neither cleared the graphs nor keyed them by initialisation: where the workspace came back at its old
    address the three calls were replays (0, 3) of the graph with the old heatfac, and hr x 1003.5 missed hr_before x 1004.0 by the whole
    5e-4 (profiles/lifecycle_tests.md)."""
    import torch
    call = _DeviceCall(hip, 1000, 72, "cloudy", idrv=1)
    prev = hip.set_graph_max(1 << 20)
    try:
        before = _capture(hip, call)
        hip.rrtmg_lw_ini(1003.5, kdata=hip.STANDIN_KDATA, device=0)
        c0, r0 = hip.graph_stats()
        after = [call.run(1) for _ in range(3)]
        c1, r1 = hip.graph_stats()
        hip.set_graph_max(0)
        plain = call.run(1)
    finally:
        hip.set_graph_max(prev)
        _as_session(hip)
    b, p = call.named(before), call.named(plain)
    worst = max(float(np.abs(call.named(a)["hr"] * 1003.5 / (b["hr"] * 1004.0) - 1.0).max()) for a in after)
    print(f"after re-init: captures, replays = {c1 - c0}, {r1 - r0}; max |hr x 1003.5 / (hr_before x 1004.0) - 1| = {worst:.3e}; "
          f"calls equal to the plain launches: {[bool(torch.equal(_bits(a), _bits(plain))) for a in after]}")
    for i, a in enumerate(after):
        assert torch.equal(_bits(a), _bits(plain)), f"call {i + 1} after the re-initialisation differs from the plain launches"
    for k in ("uflx", "dflx", "uflxc", "dflxc", "duflx_dt", "duflxc_dt"):
        assert np.array_equal(p[k], b[k]), k
    for k in ("hr", "hrc"):
        np.testing.assert_allclose(p[k] * 1003.5, b[k] * 1004.0, rtol=1e-12, atol=1e-12)
        assert not np.array_equal(p[k], b[k]), k
    assert (c1 - c0, r1 - r0) == (1, 1)
    ref = oracle.rrtmg_lw(call.ncol, call.nlay, 2, 1, call.host)
    b["icld"] = ref["icld"]
    _compare(b, ref, 1, "graph before the re-initialisation")


# -------------------------------------------------------------------------------------------- 1b. re-init under a live graph: k-data
def _scaled_kdata(path, factor=1.25):
    """the stand-in absorption coefficients with every band's major-gas tables (bNN.kao, bNN.kbo) x factor"""
    std = read_blob(STANDIN)
    scaled = {k: (v * factor if re.fullmatch(r"b\d\d\.k[ab]o", k) else v) for k, v in std.items()}
    assert sum(1 for k in std if re.fullmatch(r"b\d\d\.k[ab]o", k)) == 28
    write_blob(path, scaled)
    return std, scaled


def test_kdata_blob_round_trip(tmp_path):
    """read_blob / write_blob reproduce the stand-in file byte for byte, and the scaled file differs from it in the kao / kbo tables only."""
    std = read_blob(STANDIN)
    rt = str(tmp_path / "roundtrip.kdata.bin")
    write_blob(rt, std)
    assert os.path.getsize(rt) == os.path.getsize(STANDIN)
    assert open(rt, "rb").read() == open(STANDIN, "rb").read()
    _, scaled = _scaled_kdata(str(tmp_path / "scaled.kdata.bin"))
    back = read_blob(str(tmp_path / "scaled.kdata.bin"))
    assert os.path.getsize(str(tmp_path / "scaled.kdata.bin")) == os.path.getsize(STANDIN)
    assert list(back) == list(std)
    for k in std:
        assert back[k].dtype == std[k].dtype and back[k].shape == std[k].shape, k
        if re.fullmatch(r"b\d\d\.k[ab]o", k):
            assert np.array_equal(back[k], std[k] * 1.25) and not np.array_equal(back[k], std[k]), k
        else:
            assert np.array_equal(back[k], std[k]), k


@gpu
def test_reinit_with_other_kdata_under_a_live_graph(hip, tmp_path):
    """rrtmg_lw_ini(other absorption coefficients) while a call's graph is live: the calls that follow equal a fresh library
    (finalize, init with that file, graphs off) bit for bit and differ from the stand-in's result; back with the stand-in, the first result
    returns bit for bit.

    Before the fix, where the tables and the workspace came back at their old addresses, the three calls were replays (0, 3) of kernels
    that READ the tables through the old pointers - the new coefficients, by luck of the allocator; where the tables came back elsewhere
    the replays read freed memory (profiles/lifecycle_tests.md)."""
    import torch
    scaled = str(tmp_path / "scaled.kdata.bin")
    _scaled_kdata(scaled)
    call = _DeviceCall(hip, 1000, 72, "cloudy", idrv=1)
    prev = hip.set_graph_max(1 << 20)
    try:
        first = _capture(hip, call)
        hip.rrtmg_lw_ini(1004.0, kdata=scaled, device=0)
        c0, r0 = hip.graph_stats()
        got = [call.run(1) for _ in range(3)]
        c1, r1 = hip.graph_stats()
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=scaled, device=0)
        hip.set_graph_max(0)
        want = call.run(1)
        hip.set_graph_max(1 << 20)
        _capture(hip, call)
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        back = [call.run(1) for _ in range(3)]
    finally:
        hip.set_graph_max(prev)
        _as_session(hip)
    print(f"after re-init with scaled k-data: captures, replays = {c1 - c0}, {r1 - r0}; max |d| to the fresh library = "
          f"{max(float((g - want).abs().max()) for g in got):.3e}, to the stand-in result = {float((want - first).abs().max()):.3e}")
    assert torch.isfinite(want).all()
    assert float((want - first).abs().max()) > 1e-3            # (other coefficients, other fluxes)
    for i, g in enumerate(got):
        assert torch.equal(_bits(g), _bits(want)), f"call {i + 1} after init with the scaled coefficients"
    for i, g in enumerate(back):
        assert torch.equal(_bits(g), _bits(first)), f"call {i + 1} after init with the stand-in again"
    assert (c1 - c0, r1 - r0) == (1, 1)


# -------------------------------------------------------------------------------------------- 1c. history independence
class _Probes:
    """The fixed set of small calls whose results must not depend on what the library did before: a graph-eligible device call, a host call
    with aerosol and d/dT, a fused McICA call (kissvec), gas optics, a spectral host call - all of 40 layers, so that the workspace
    keeps its shape and the device call's graph can stay alive from one round to the next."""
    NLAY = 40

    def __init__(self, hip):
        self.hip = hip
        self.dev = _DeviceCall(hip, 300, self.NLAY, "cloudy", idrv=0, col0=11)
        self.aer = make_gcm_inputs(200, self.NLAY, "aer_idrv", col0=23)
        self.cld = make_gcm_inputs(150, self.NLAY, "cloudy", col0=31)
        self.spec = make_gcm_inputs(130, self.NLAY, "cloudy", col0=47)

    def run(self):
        hip, res = self.hip, {}
        for k, v in self.dev.named(self.dev.run(1)).items():
            res["device." + k] = v
        a = hip.rrtmg_lw_from_dict(self.aer, icld=2, idrv=1)
        res.update({"host." + k: a[k] for k in OUT6 + ("duflx_dt", "duflxc_dt")})
        m = hip.rrtmg_lw_mcica_subcol_from_dict(self.cld, 140, 0, icld=2)
        res.update({"mcica." + k: m[k] for k in OUT6})
        g = hip.gas_optics(self.aer, idrv=1)
        res.update({"optics." + k: g[k] for k in ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt")})
        s = hip.rrtmg_lw_from_dict(self.spec, icld=2, out=_nan_out(130, self.NLAY), spectral=True)
        res.update({"spectral." + k: s[k] for k in OUT6 + ("uflxs", "dflxs", "uflxcs", "dflxcs")})
        return {k: np.array(v, copy=True) for k, v in res.items()}

    def check_against_oracle(self, oracle, res):
        from test_hip_optics import RTOL, _err
        pick = lambda p: {k[len(p):]: v for k, v in res.items() if k.startswith(p)}
        ref = oracle.rrtmg_lw(300, self.NLAY, 2, 0, self.dev.host)
        _compare(dict(pick("device."), icld=ref["icld"]), ref, 0, "probe: device call")
        ref = oracle.rrtmg_lw(200, self.NLAY, 2, 1, self.aer)
        _compare(dict(pick("host."), icld=ref["icld"]), ref, 1, "probe: host call")
        d = self.cld
        sub = oracle.mcica_subcol(150, self.NLAY, 2, 140, 0, d["play"], d["cldfr"], d["cicewp"], d["cliqwp"], d["reice"], d["reliq"], d["taucld"],
                                  np.zeros((150, self.NLAY)))
        dd = dict(d)
        dd.update({k: sub[k] for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "taucmcl")})
        ref = oracle.rrtmg_lw(150, self.NLAY, 2, 0, dd, mcica=True)
        _compare(dict(pick("mcica."), icld=ref["icld"]), ref, 0, "probe: fused McICA call")
        for i in (0, 99, 199):
            col = oracle.column(inatm(self.aer, i, 0))
            for k in ("taug", "fracs"):
                assert _err(res["optics." + k][i], col[k], RTOL) <= 1.0, (k, i)
        ref = oracle.rrtmg_lw(130, self.NLAY, 2, 0, self.spec)
        _compare(dict(pick("spectral."), icld=ref["icld"]), ref, 0, "probe: spectral host call")
        _check_sums(pick("spectral."), "probe: spectral host call")


def _same(got, base):
    """names of the output arrays that differ from the baseline in any bit"""
    return [k for k in base if not (got[k].shape == base[k].shape and np.array_equal(got[k].view(np.int64), base[k].view(np.int64)))]


class _Ops:
    """The operations of the sequence test.  Each leaves the library as the session fixture made it; those that hold a switch or a batch
    size for a while run the probes under it as well (results are documented not to depend on either)."""

    def __init__(self, hip, probes, base, rng):
        self.hip, self.probes, self.base, self.rng = hip, probes, base, rng
        self.grown = 2000
        self.cloudy = make_gcm_inputs(64, _Probes.NLAY, "cloudy", col0=3)

    def _probes_hold(self, what):
        bad = _same(self.probes.run(), self.base)
        assert not bad, f"{what}: {bad} differ from the fresh library's"

    def reinit_same(self):
        self.hip.rrtmg_lw_ini(1004.0, kdata=self.hip.STANDIN_KDATA, device=0)

    def reinit_cpdair_and_back(self):
        self.hip.rrtmg_lw_ini(1003.5, kdata=self.hip.STANDIN_KDATA, device=0)
        try:
            self.probes.dev.run(3)               # (a graph with the other heatfac)
        finally:
            self.hip.rrtmg_lw_ini(1004.0, kdata=self.hip.STANDIN_KDATA, device=0)

    def three_devices_and_back(self):
        try:
            self.hip.init_devices([0, 0, 0], kdata=self.hip.STANDIN_KDATA)
            assert self.hip.num_devices() == 3
            self._probes_hold("three virtual devices")
        finally:
            self.hip.rrtmg_lw_ini(1004.0, kdata=self.hip.STANDIN_KDATA, device=0)
        assert self.hip.num_devices() == 1

    def g256_and_back(self):
        self.hip.select_gpoints(256)
        try:
            self.hip.rrtmg_lw_ini(1004.0, kdata=self.hip.STANDIN_KDATA, device=0)
            got = self.hip.rrtmg_lw_from_dict(self.cloudy)
            assert np.isfinite(got["uflx"]).all()
            self.hip.finalize(selected_only=True)
        finally:
            self.hip.select_gpoints(140)

    def batch_and_back(self):
        n = int(self.rng.integers(64, 513)) if self.rng.random() < 0.5 else int(self.rng.integers(64, 1048577))
        try:
            self.hip.set_batch(n)
            self._probes_hold(f"set_batch({n})")
        finally:
            self.hip.set_batch(0)

    def workspace_grows(self):
        self.grown += 700
        d = make_gcm_inputs(self.grown, _Probes.NLAY, "cloudy", col0=5)
        before = self.hip.workspace_bytes()
        got = self.hip.rrtmg_lw_from_dict(d)
        assert np.isfinite(got["uflx"]).all() and self.hip.workspace_bytes() > before

    def device_probe_three_times(self):
        for _ in range(3):                       # (plain, capture, replay - or replays, where the graph is still alive)
            got = self.probes.dev.named(self.probes.dev.run(1))
            bad = [k for k in got if not np.array_equal(got[k], self.base["device." + k])]
            assert not bad, bad

    def switches_and_back(self):
        hip, rng = self.hip, self.rng
        prev_one = hip.set_one_sweep_max(int(rng.choice([0, 1 << 30])))
        prev_min = hip.column_sort_min()
        prev_sort = hip.set_column_sort(bool(rng.integers(0, 2)), int(rng.choice([0, 24, 1 << 24])))
        prev_wide = hip.set_wide_window(int(rng.integers(0, 2)))
        try:
            self._probes_hold("tuning switches")
        finally:
            hip.set_one_sweep_max(prev_one)
            hip.set_column_sort(prev_sort, prev_min)
            hip.set_wide_window(prev_wide)

    def argument_error(self):
        d = self.cloudy
        with pytest.raises(self.hip.RrtmgLwError, match="needs alpha"):
            self.hip.mcica_subcol_lw(64, _Probes.NLAY, 5, 140, 0, d["play"], d["cldfr"], d["cicewp"], d["cliqwp"], d["reice"], d["reliq"], d["taucld"])

    def physics_error(self):
        d = dict(self.cloudy)
        d["reice"] = np.asfortranarray(np.full((64, _Probes.NLAY), 500.0))
        with pytest.raises(self.hip.RrtmgLwError, match="ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS"):
            self.hip.rrtmg_lw_from_dict(d)

    def finalize_and_init(self):
        self.hip.finalize()
        self.hip.rrtmg_lw_ini(1004.0, kdata=self.hip.STANDIN_KDATA, device=0)

    NAMES = ("reinit_same", "reinit_cpdair_and_back", "three_devices_and_back", "g256_and_back", "batch_and_back", "workspace_grows",
             "device_probe_three_times", "switches_and_back", "argument_error", "physics_error", "finalize_and_init")


@gpu
@pytest.mark.parametrize("seed", [20241017])
def test_results_do_not_depend_on_what_came_before(hip, oracle, seed):
    """A column's result depends on its inputs and the tables, on nothing else: after every operation of a seeded sequence (every kind at
    least once, forty in all) the probe calls give, bit for bit, what they gave in a fresh library with the graphs off - which is checked
    against the oracle once, at the bars of the other tests."""
    probes = _Probes(hip)
    prev = hip.set_graph_max(0)
    try:
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        base = probes.run()
    finally:
        hip.set_graph_max(prev)
    probes.check_against_oracle(oracle, base)
    rng = np.random.default_rng(seed)
    ops = _Ops(hip, probes, base, rng)
    seq = [str(s) for s in rng.permutation(_Ops.NAMES)] + [str(s) for s in rng.choice(_Ops.NAMES, 40 - len(_Ops.NAMES))]
    c0, r0 = hip.graph_stats()
    replays = 0
    try:
        for i, name in enumerate(seq):
            where = f"operation {i} ({name}) after {seq[:i]}"
            try:
                getattr(ops, name)()
            except Exception as e:
                raise AssertionError(f"{where}: {e}") from e
            _, ra = hip.graph_stats()
            bad = _same(probes.run(), base)
            _, rb = hip.graph_stats()
            replays += rb - ra
            assert not bad, f"{where}: the probes' {bad} differ from the fresh library's"
            assert hip.gpoints() == 140 and hip.num_devices() == 1 and hip.effective_batch(72) == 262144, where
    finally:
        _as_session(hip)
    print(f"{len(seq)} operations, {replays} of the device probes after them replayed from a graph")
    assert replays >= 3             # (the sequence does exercise the graph cache: about ten expected from the order of its operations)


# -------------------------------------------------------------------------------------------- 1d. rows past 2^31 bytes
def _balanced(ncol, cap):
    """columns of the largest batch (driver.hip: balanced_batch)"""
    if ncol <= cap:
        return ncol
    nbatch = -(-ncol // cap)
    return min((-(-ncol // nbatch) + 255) // 256 * 256, cap)


def _tile_to_device(torch, a, cax, reps, dev):
    """the numpy array `a` (column axis cax) repeated `reps` times along its columns, in HBM, stored column-fastest"""
    nd = a.ndim
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(*reversed(range(nd))))).to(dev)
    rep = [1] * nd
    rep[nd - 1 - cax] = reps
    t = t.repeat(*rep)
    return t.permute(*reversed(range(nd))) if nd > 1 else t


@gpu
def test_workspace_rows_past_two_gib(hip, oracle):
    """One maximum-random-overlap batch whose cloudy levels read workspace rows that begin 2^31 bytes and more behind their array's start.

    Arrays the sweeps address by a scalar row offset (kernels.hip: bload_*(.., soff), the direct raw_buffer_load sites included), with the
    bytes per column and level (n = columns of the workspace, L = layers):
        rtrnmr's overlap factors  W.ovl    (lev x 3 + 0..2) x 16 n   lev = 0..L   mode 2       ends at 48 (L + 1) n
        sub-column fraction / emissivity   W.cfef   lev x 32 n       lev < L      mode 3       ends at 32 L n
        cell codes                scr[]    lev x 16 n                lev < L      every mode   ends at 16 L n
        rtrn's emissivity term    W.efcl   lev x 8 n                 lev < L      mode 1
        cloud flags               cflag    (lev + 1) x 4 n           lev < L      cloudy modes
        binary-key words          fw       lev x 4 n                 lev < L      every mode
    The overlap factors reach the range first.  Smallest shape: a cloudy level l reads the rows from 48 l n on, l <= L, so L n >= 2^31 / 48 =
    44.7e6 - the workspace is proportional to L n, every such shape costs the same; 200 layers x 230 400 columns under set_batch(262144)
    put the rows of the layers 195 .. 200 past 0x7ffffff0.  Clouds are set in the top four layers of half the columns (the `toplayer`
    construction of test_special_cloud_configurations; only cloudy levels use what they read from those rows, and the synthetic decks stop
    at layer 14).  Reference: windows of 300 of the same columns in stand-alone calls made BEFORE the large one in a fresh library (the
    row stride is the workspace's width, which a call of the same layers inherits), bit for bit; the oracle on the middle window.

    McICA's sub-column arrays (mode 3, cfef: 32 L n) cannot be brought there on one MI355X: L n >= 67.1e6 cells, for each of which the
    caller's four sub-column arrays alone hold 140 x 4 x 8 = 4 480 bytes - 300 GB before any workspace.

    Before the fix eff_batch kept the offsets below 2^32 only and this call was one batch of 230 400 columns; now it is two of 115 200
    (profiles/lifecycle_tests.md)."""
    import torch
    from rrtmg_lw_amd.shard import output_rows, output_views
    nlay, nbase, reps, batch = 200, 1024, 225, 262144
    ncol = nbase * reps
    top = 4
    base = make_gcm_inputs(nbase, nlay, "cloudy", col0=55)
    rng = np.random.default_rng(7)
    crowned = rng.random(nbase) < 0.5
    cf = np.array(base["cldfr"])
    cf[:, nlay - top:] = np.where(crowned, 0.6, 0.0)[:, None]
    base["cldfr"] = np.asfortranarray(cf)
    for k in ("cliqwp", "cicewp"):
        a = np.array(base[k])
        a[:, nlay - top:] = np.where(crowned, 20.0, 0.0)[:, None]
        base[k] = np.asfortranarray(a)
    # the shape arithmetic: at least one cloudy (column, level) reads a row that begins past the descriptor's range
    nb = _balanced(ncol, batch)
    cloudy_levels = np.nonzero((cf > 0).any(axis=0))[0] + 1
    first_row = int(cloudy_levels.max()) * 3 * 16 * nb
    print(f"{ncol} columns x {nlay} layers, requested batch {batch}: {nb} columns per batch, the overlap rows of layer {cloudy_levels.max()} begin at "
          f"{first_row} = {first_row / 2 ** 31:.3f} x 2^31")
    assert first_row >= SWEEP_RANGE and crowned.sum() > 100

    def window(c0, n):
        idx = (c0 + np.arange(n)) % nbase
        dn = dict(base, ncol=n)
        for k, v in base.items():
            if isinstance(v, np.ndarray):
                dn[k] = np.asfortranarray(v[:, idx, :] if k == "taucld" else v[idx])
        return dn, crowned[idx]

    dev = torch.device("cuda", 0)
    inputs = sum(v.nbytes for v in base.values() if isinstance(v, np.ndarray)) * reps
    needed = 2048 * nb * nlay + inputs + 8 * output_rows(nlay, 0) * ncol + (4 << 30)        # (README: about 2 kB of workspace per column and layer)
    free, total = torch.cuda.mem_get_info(dev)
    if free < needed:
        pytest.skip(f"needs {needed} bytes of device memory, {free} of {total} are free")
    windows = [(0, 300), (ncol // 2 - 150, 300), (ncol - 300, 300)]
    try:
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        alone = []
        for c0, n in windows:
            dn, cr = window(c0, n)
            assert cr.sum() > 50
            alone.append((dn, hip.rrtmg_lw_from_dict(dn)))
        small_ws = hip.workspace_bytes()
        d = dict(base, ncol=ncol)
        for k, v in base.items():
            if isinstance(v, np.ndarray):
                d[k] = _tile_to_device(torch, v, 1 if k == "taucld" else 0, reps, dev)
        outbuf = torch.full((output_rows(nlay, 0), ncol), float("nan"), dtype=torch.float64, device=dev)
        out = output_views(outbuf, nlay, 0)
        s = torch.cuda.current_stream().cuda_stream
        hip.set_batch(batch)
        eff = hip.effective_batch(nlay)
        hip.rrtmg_lw_device(d, out, stream=s)
        hip.check(s)
        print(f"workspace_bytes() = {hip.workspace_bytes()} after the call ({small_ws} after the stand-alone windows), effective batch {eff}")
        for k in OUT6:
            assert torch.isfinite(out[k]).all(), k
        worst = 0.0
        for (c0, n), (dn, ref) in zip(windows, alone):
            for k in OUT6:
                got = out[k][:, c0:c0 + n].t().cpu().numpy()
                diff = float(np.abs(got - ref[k]).max())
                worst = max(worst, diff)
                print(f"window {c0}: max |d {k}| = {diff:.3e}, {int((got != ref[k]).any(axis=1).sum())} of {n} columns differ")
        print(f"largest difference to the stand-alone calls: {worst:.3e}")
        for (c0, n), (dn, ref) in zip(windows, alone):
            for k in OUT6:
                assert np.array_equal(out[k][:, c0:c0 + n].t().cpu().numpy(), ref[k]), (k, c0)
    finally:
        d = out = outbuf = None
        hip.finalize()                  # (the workspace of this call is of no use to the tests that follow)
        torch.cuda.empty_cache()
        _as_session(hip)
    dn, got = alone[1]
    ref = oracle.rrtmg_lw(300, nlay, 2, 0, dn)
    assert np.abs(ref["dflx"] - ref["dflxc"])[:, nlay - top].max() > 1.0            # the crowns matter where they are
    print(f"middle window against the oracle: max |dflux| = {max(np.abs(got[k] - ref[k]).max() for k in ('uflx', 'dflx', 'uflxc', 'dflxc')):.3e}, "
          f"max |dhr| over all layers = {max(np.abs(got[k] - ref[k]).max() for k in ('hr', 'hrc')):.3e}")
    _compare_thin_layers(got, ref, dn, 0, "middle window, stand-alone")


# -------------------------------------------------------------------------------------------- 2. the batch size in force
def _last_byte(nlay, n):
    """end of the last row the sweeps can address by row offset in a workspace n columns wide (see test_workspace_rows_past_two_gib): the
    largest over the arrays of every mode, from the layout alone"""
    ends = {"ovl": ((nlay * 3 + 2) * 16 + 16) * n, "cfef": ((nlay - 1) * 32 + 32) * n, "codes": ((nlay - 1) * 16 + 16) * n,
            "efcl": ((nlay - 1) * 8 + 8) * n, "cflag": ((nlay - 1 + 1) * 4 + 4) * n, "fw": ((nlay - 1) * 4 + 4) * n}
    assert max(ends, key=ends.get) == "ovl"
    return max(ends.values())


@gpu
def test_effective_batch(hip):
    """The batch size in force: by the call's layers by default (72 -> 262 144, 137 -> 131 072, 200 -> 65 536); a size named with set_batch
    is halved until every row the sweeps address by offset ends inside the 0x7ffffff0 bytes of their descriptors - but no further; and
    set_batch(0) brings the defaults back."""
    hip.set_batch(0)
    defaults = {72: 262144, 96: 262144, 137: 131072, 200: 65536}
    try:
        for nlay, b in defaults.items():
            assert hip.effective_batch(nlay) == b, nlay
            assert _last_byte(nlay, b) <= SWEEP_RANGE
        for named, nlay in ((262144, 603), (262144, 200), (262144, 169), (262144, 170), (1048576, 72), (1048576, 603), (300, 603), (70000, 603)):
            hip.set_batch(named)
            b = hip.effective_batch(nlay)
            print(f"set_batch({named}), {nlay} layers: {b} columns per batch, last row ends at {_last_byte(nlay, b) / SWEEP_RANGE:.3f} of the range")
            assert 64 <= b <= named
            assert _last_byte(nlay, b) <= SWEEP_RANGE, (named, nlay, b)
            assert b == named or _last_byte(nlay, 2 * b) > SWEEP_RANGE, (named, nlay, b)       # halved, and not once more than needed
        hip.set_batch(262144)
        assert hip.effective_batch(169) == 262144 and hip.effective_batch(170) == 131072
    finally:
        hip.set_batch(0)
    for nlay, b in defaults.items():
        assert hip.effective_batch(nlay) == b, nlay


# -------------------------------------------------------------------------------------------- 3. init .. finalize, over and over
ENOTINIT = 4


def _raw(v):
    """the bytes of an output, whatever holds it"""
    return (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)).tobytes()


class _Families:
    """One call per family of GPU resources (driver.hip: device buffers, pinned buffers, streams, events, graphs) at 130 columns x 20 layers
    - a ragged window, a partial 64-column block - cloudy, idrv = 1.  The arrays are made once; a cycle only calls."""
    NCOL, NLAY = 130, 20

    def __init__(self, hip):
        import torch
        from rrtmg_lw_amd import arrays
        self.hip, self.torch, self.arrays = hip, torch, arrays
        n, L = self.NCOL, self.NLAY
        self.dev = _DeviceCall(hip, n, L, "cloudy", idrv=1, col0=0)
        self.tall = _DeviceCall(hip, n, 72, "cloudy", idrv=1, col0=0)
        self.host = dict(make_gcm_inputs(n, L, "cloudy"), inflglw=2)
        self.chunks = [make_gcm_inputs(70, L, "cloudy", col0=0), make_gcm_inputs(60, L, "cloudy", col0=70)]
        self.form = arrays.ArrayForm(4, 1, 1)
        x = arrays.from_reference(self.host, self.form)
        self.formed = {k: (torch.from_numpy(v).to("cuda:0") if isinstance(v, np.ndarray) else v) for k, v in x.items()}

    def cycle(self):
        """-> (outputs by name, [(workspace_bytes, effective_batch(20)) after every call], [graph_stats deltas])"""
        hip, torch = self.hip, self.torch
        res, marks, graphs = {}, [], []
        s = torch.cuda.current_stream().cuda_stream

        def mark():
            marks.append((hip.workspace_bytes(), hip.effective_batch(self.NLAY)))

        def keep(tag, out, names):
            res.update({tag + "." + k: _raw(out[k]) for k in names})
        flux = OUT6 + ("duflx_dt", "duflxc_dt")
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        mark()
        c0, r0 = hip.graph_stats()
        res["device"] = _raw(self.dev.run(3))                            # plain launches, capture, replay
        c1, r1 = hip.graph_stats()
        graphs.append((c1 - c0, r1 - r0))
        mark()
        keep("host", hip.rrtmg_lw_from_dict(self.host, icld=2, idrv=1), flux)           # copy streams, host sets, h_tot
        mark()
        for irng in (0, 1):                                              # mask, kiss table / MT states, d_rnd
            keep(f"fused{irng}", hip.rrtmg_lw_mcica_subcol_from_dict(self.host, 11, irng, icld=2, idrv=1), flux)
            mark()
        keep("optics", hip.gas_optics(self.host, idrv=1), ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt"))
        mark()
        out = self.arrays.empty_like_form(flux, self.NCOL, self.NLAY, self.form, device="cuda:0", fill=float("nan"))
        hip.rrtmg_lw_device(self.formed, out, icld=2, idrv=1, stream=s, form=self.form)      # form staging
        hip.check(s)
        keep("as", out, flux)
        mark()
        q = hip.ChunkQueue(self.NLAY, 2, 1, 2, self.host["iceflglw"], self.host["liqflglw"])        # Q.pinned
        outs = [q.add(c) for c in self.chunks]
        q.flush()
        for i, o in enumerate(outs):
            keep(f"queue{i}", o, flux)
        mark()
        buf = ctypes.create_string_buffer(1 << 16)
        hip.lib().rrtmg_lw_hip_profile_begin()                           # the event pool
        try:
            res["profiled"] = _raw(self.dev.run(1))
        finally:
            hip.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
        res["profiled.kernels"] = " ".join(sorted(ln.split()[0] + "x" + ln.split()[1] for ln in buf.value.decode().splitlines() if ln.strip()))
        mark()
        c0, r0 = hip.graph_stats()
        res["tall"] = _raw(self.tall.run(1))                             # 72 layers: the workspace dropped and rebuilt, the graphs cleared
        res["device.again"] = _raw(self.dev.run(2))                      # (back at 20 layers: plain, then captured anew)
        c1, r1 = hip.graph_stats()
        graphs.append((c1 - c0, r1 - r0))
        mark()
        hip.finalize()
        assert hip.num_devices() == 0
        with pytest.raises(hip.RrtmgLwError, match=f"error {ENOTINIT}: rrtmg_lw_hip_init has not been called"):
            hip.rrtmg_lw_device(self.dev.d, self.dev.out, icld=2, idrv=1, stream=s)
        return res, marks, graphs


@gpu
def test_three_cycles_of_init_and_finalize(hip):
    """rrtmg_lw_ini, one call per resource family, finalize - three times in one process.  Every cycle gives the outputs of the first bit
    for bit, holds the same device memory (workspace_bytes) and batch size after every call, and captures and replays the same number of
    graphs; after every finalize the library is uninitialised (num_devices() == 0, a call is refused with RRTMG_LW_HIP_ENOTINIT)."""
    fam = _Families(hip)
    try:
        hip.finalize()
        first = fam.cycle()
        res, marks, graphs = first
        print(f"cycle 1: {len(res)} outputs, workspace_bytes after each call {[m[0] for m in marks]}, graph captures / replays {graphs}")
        assert res["device"] == res["profiled"] == res["device.again"]          # (graph replay, profiled launches, plain launches: one result)
        assert all(np.isfinite(np.frombuffer(v, dtype=np.float32 if k.startswith("as.") else np.float64)).all()
                   for k, v in res.items() if k != "profiled.kernels")
        assert "k_layer" in res["profiled.kernels"] and graphs[0][0] == 1 and graphs[0][1] >= 1 and graphs[1] == (1, 0)
        assert marks[-1][0] > marks[1][0] > marks[0][0] >= 0
        for n in (2, 3):
            res, marks, graphs = fam.cycle()
            bad = [k for k in first[0] if res[k] != first[0][k]]
            assert not bad, f"cycle {n}: {bad} differ from cycle 1"
            assert marks == first[1], f"cycle {n}: workspace_bytes / effective_batch {marks} against {first[1]}"
            assert graphs == first[2], f"cycle {n}: graph captures / replays {graphs} against {first[2]}"
    finally:
        _as_session(hip)


_CHILD = """
import ctypes, sys
import numpy as np
import torch
from rrtmg_lw_amd import api
from rrtmg_lw_amd.shard import output_rows, output_views
from rrtmg_lw_amd.synth import make_gcm_inputs
api.rrtmg_lw_ini(1004.0, kdata=api.STANDIN_KDATA, device=0)
dev = torch.device("cuda", 0)
d = make_gcm_inputs(64, 20, "cloudy", backend="torch", device=dev)
buf = torch.full((output_rows(20, 0), 64), float("nan"), dtype=torch.float64, device=dev)
out = output_views(buf, 20, 0)
s = torch.cuda.current_stream().cuda_stream
api.rrtmg_lw_device(d, out, icld=2, idrv=0, stream=s)
api.check(s)
assert torch.isfinite(buf).all()
h = api.rrtmg_lw_from_dict(make_gcm_inputs(64, 20, "cloudy"))
assert np.isfinite(h["uflx"]).all()
names = ctypes.create_string_buffer(1 << 16)
api.lib().rrtmg_lw_hip_profile_begin()
api.rrtmg_lw_device(d, out, icld=2, idrv=0, stream=s)
api.check(s)
api.lib().rrtmg_lw_hip_profile_end(names, len(names))
assert b"k_layer" in names.value
for _ in range(int(sys.argv[1])):
    api.finalize()
print("child: ok", flush=True)
"""


@gpu
@pytest.mark.parametrize("finalizes", [0, 2], ids=["exit without finalize", "finalize twice"])
def test_a_process_may_end_without_finalize(finalizes):
    """A fresh process initialises, makes a device call, a host call and a profiled call of 64 x 20 columns and ends - without
    rrtmg_lw_hip_finalize (as Python tests and host models do: the library's globals hold streams, events and buffers then, and nothing
    of it may call into the HIP runtime from a static destructor), or after finalizing twice (the second is a no-op).  Return code 0 and
    nothing on stderr either way."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONWARNINGS="ignore")
    p = subprocess.run([sys.executable, "-c", _CHILD, str(finalizes)], timeout=120, capture_output=True, text=True, cwd=root, env=env)
    print(f"return code {p.returncode}; stdout {p.stdout!r}; stderr {p.stderr!r}")
    assert p.returncode == 0 and "child: ok" in p.stdout
    # (libdrm's complaint about its missing table of marketing names, where the file is not installed, is no word of the runtime's)
    said = [ln for ln in p.stderr.splitlines() if ln.strip() and not ln.rstrip().endswith("amdgpu.ids: No such file or directory")]
    assert not said, said
