"""Every path through the driver's launch layer still launches - with the sweeps' dynamic-LDS limit raised for the instantiation it
reaches: k_sweepc and k_sweepz need more than the 64 KB a kernel gets without asking, so one that ensure_sweep_attrs leaves out fails
at launch - and still agrees with its neighbours.  test_one_band_per_workgroup_is_transparent, the one-sweep cases of test_hip_parity.py
and test_hip_spectral.py pin each switch on its own; this is the matrix of their combinations:

  entry    the device non-McICA entry with icld 0 (k_sweepc<., 0> alone), 1 (rtrn) and 2 (rtrnmr), the device McICA entry with explicit
           sub-column arrays (k_sweepz<., 3>), the fused generator + solver entry (the generator's mask: k_sweepz<., 4>)
  idrv     0, 1
  spectral no, yes (the SPEC instantiations)
  sweeps   three launches, one launch (the cloud-zone kernel over all levels), and each of the two with one band per workgroup

No combination of these is refused by the library, so none is left out.  130 columns are two full 64-column blocks and a ragged one of
2; the ragged block and a few other columns hold no cloud.  Every comparison is bit for bit.  The kernel names of one profiled call per
entry were recorded from the commit before the launch layer was rewritten (an MI355X, the 140-g-point library) and are literals here.
"""
import ctypes

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

NCOL, NLAY = 130, 20
CLOUD_FREE = (5, 64, 65, 66, 127, 128, 129)
BROAD = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
DDT = ("duflx_dt", "duflxc_dt")
SPEC = ("uflxs", "dflxs", "uflxcs", "dflxcs")
ENTRIES = ("nomcica icld0", "nomcica icld1", "nomcica icld2", "mcica arrays", "fused mask")
# (one_sweep_max, split_max); the first is the reference of every comparison
PATHS = {"three launches": (0, 0), "one launch": (1 << 30, 0),
         "one band per workgroup, three launches": (0, 1 << 20), "one band per workgroup, one launch": (1 << 30, 1 << 20)}

# kernel names of one profiled call (idrv 0, not spectral, three launches) per entry, as recorded from the parent commit
KERNELS = {
    "nomcica icld0": {
        "k_colprep", "k_flux", "k_layer<clear,0>", "k_layer<clear,1>", "k_sweepc<1,0>", "k_sweepc<2,0>", "k_sweepc<3,0>",
        "k_sweepc<4,0>"
    },
    "nomcica icld1": {
        "k_blocksort", "k_cloudlay", "k_cloudscan", "k_colprep", "k_colsort", "k_flux", "k_layer<cloud,0>",
        "k_layer<cloud,1>", "k_sweepc<1,0>", "k_sweepc<1,1>", "k_sweepc<1,2>", "k_sweepc<2,0>", "k_sweepc<2,1>",
        "k_sweepc<2,2>", "k_sweepc<3,0>", "k_sweepc<3,1>", "k_sweepc<3,2>", "k_sweepc<4,0>", "k_sweepc<4,1>", "k_sweepc<4,2>",
        "k_sweepz<1,1>", "k_sweepz<2,1>", "k_sweepz<3,1>", "k_sweepz<4,1>"
    },
    "nomcica icld2": {
        "k_blocksort", "k_cloudlay", "k_cloudscan", "k_colprep", "k_colsort", "k_flux", "k_layer<cloud,0>",
        "k_layer<cloud,1>", "k_sweepc<1,0>", "k_sweepc<1,1>", "k_sweepc<1,2>", "k_sweepc<2,0>", "k_sweepc<2,1>",
        "k_sweepc<2,2>", "k_sweepc<3,0>", "k_sweepc<3,1>", "k_sweepc<3,2>", "k_sweepc<4,0>", "k_sweepc<4,1>", "k_sweepc<4,2>",
        "k_sweepz<1,2>", "k_sweepz<2,2>", "k_sweepz<3,2>", "k_sweepz<4,2>"
    },
    "mcica arrays": {
        "k_blocksort", "k_cloudmc<arrays>", "k_colprep", "k_flux", "k_layer<mcica,0>", "k_layer<mcica,1>", "k_sweepc<1,0>",
        "k_sweepc<1,1>", "k_sweepc<1,2>", "k_sweepc<2,0>", "k_sweepc<2,1>", "k_sweepc<2,2>", "k_sweepc<3,0>", "k_sweepc<3,1>",
        "k_sweepc<3,2>", "k_sweepc<4,0>", "k_sweepc<4,1>", "k_sweepc<4,2>", "k_sweepz<1,3>", "k_sweepz<2,3>", "k_sweepz<3,3>",
        "k_sweepz<4,3>"
    },
    "fused mask": {
        "k_blocksort", "k_cloudmc<mask>", "k_colprep", "k_colsort", "k_flux", "k_layer<mcmask,0>", "k_layer<mcmask,1>",
        "k_subcol_kiss", "k_sweepc<1,0>", "k_sweepc<1,1>", "k_sweepc<1,2>", "k_sweepc<2,0>", "k_sweepc<2,1>", "k_sweepc<2,2>",
        "k_sweepc<3,0>", "k_sweepc<3,1>", "k_sweepc<3,2>", "k_sweepc<4,0>", "k_sweepc<4,1>", "k_sweepc<4,2>", "k_sweepz<1,4>",
        "k_sweepz<2,4>", "k_sweepz<3,4>", "k_sweepz<4,4>"
    },
}

_cache = {}


def _to_device(torch, dev, v):
    """a host array of the interface (Fortran order) as the column-fastest tensor the device entries take"""
    if not isinstance(v, np.ndarray):
        return v
    t = torch.from_numpy(np.ascontiguousarray(v.transpose())).to(dev)
    return t.permute(*reversed(range(t.dim())))


def _inputs(oracle):
    """(host dict, device dict, device sub-column arrays): computed once, never written to"""
    if not _cache:
        import torch
        dev = torch.device("cuda", 0)
        dn = make_gcm_inputs(NCOL, NLAY, "cloudy")
        for k in ("cldfr", "cliqwp", "cicewp"):
            a = np.array(dn[k], order="F")
            a[list(CLOUD_FREE)] = 0.0
            dn[k] = a
        assert (np.asarray(dn["cldfr"]) > 0).any(axis=1).sum() >= 32        # (the other columns keep their clouds)
        sc = oracle.mcica_subcol(NCOL, NLAY, 2, 140, 0, dn["play"], dn["cldfr"], dn["cicewp"], dn["cliqwp"], dn["reice"], dn["reliq"],
                                 dn["taucld"], np.zeros((NCOL, NLAY)))
        sub = {k: torch.from_numpy(np.ascontiguousarray(sc[k].transpose(2, 1, 0))).to(dev) for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "taucmcl")}
        sub.update({k: torch.from_numpy(np.ascontiguousarray(sc[k].T)).to(dev) for k in ("reicmcl", "relqmcl")})
        _cache.update(dn=dn, d={k: _to_device(torch, dev, v) for k, v in dn.items()}, sub=sub, torch=torch, dev=dev)
    return _cache


def run(hip, oracle, entry, idrv, spectral):
    """one call of `entry`; the outputs, prefilled with NaN, as host arrays"""
    c = _inputs(oracle)
    torch, d = c["torch"], c["d"]
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=c["dev"])
    o = {k: z(NLAY + 1, NCOL) for k in ("uflx", "dflx", "uflxc", "dflxc") + (DDT if idrv else ())}
    o.update(hr=z(NLAY, NCOL), hrc=z(NLAY, NCOL))
    if spectral:
        o.update({k: z(16, NLAY + 1, NCOL) for k in SPEC})
    stream = torch.cuda.current_stream().cuda_stream
    if entry.startswith("nomcica"):
        hip.rrtmg_lw_device(d, o, icld=int(entry[-1]), idrv=idrv, stream=stream)
    elif entry == "mcica arrays":
        hip.rrtmg_lw_mcica_device(d, c["sub"], o, icld=2, idrv=idrv, stream=stream)
    else:
        hip.rrtmg_lw_mcica_subcol_device(d, o, 140, 0, icld=2, idrv=idrv, stream=stream)
    hip.check(stream)
    return {k: v.cpu().numpy().T for k, v in o.items()}


def matrix(hip, oracle, entry, idrv):
    """{(path, spectral): outputs} of one (entry, idrv); the switches are put back"""
    prev_one, prev_split = hip.set_one_sweep_max(0), hip.set_split_max(0)
    try:
        runs = {}
        for path, (one, split) in PATHS.items():
            hip.set_one_sweep_max(one)
            hip.set_split_max(split)
            for spectral in (False, True):
                runs[path, spectral] = run(hip, oracle, entry, idrv, spectral)
        return runs
    finally:
        hip.set_one_sweep_max(prev_one)
        hip.set_split_max(prev_split)


def profiled(hip, oracle, entry):
    """the kernel names of one call on the three-launch path"""
    prev_one, prev_split = hip.set_one_sweep_max(0), hip.set_split_max(0)
    buf = ctypes.create_string_buffer(1 << 16)
    try:
        hip.lib().rrtmg_lw_hip_profile_begin()
        try:
            run(hip, oracle, entry, 0, False)
        finally:
            hip.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
    finally:
        hip.set_one_sweep_max(prev_one)
        hip.set_split_max(prev_split)
    return {ln.split()[0] for ln in buf.value.decode().splitlines() if ln.strip()}


@pytest.mark.parametrize("idrv", [0, 1])
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_path_gives_the_same_bits(hip, oracle, entry, idrv):
    runs = matrix(hip, oracle, entry, idrv)
    ref = runs["three launches", False]
    names = BROAD + (DDT if idrv else ())
    for k in names:
        assert np.isfinite(ref[k]).all(), (entry, idrv, k, "values left unwritten")
    for (path, spectral), got in runs.items():
        for k in names:
            assert np.array_equal(got[k], ref[k]), (entry, idrv, path, spectral, k)
    spec = runs["three launches", True]
    for k in SPEC:
        assert np.isfinite(spec[k]).all(), (entry, idrv, k, "values left unwritten")
        for path in PATHS:
            assert np.array_equal(runs[path, True][k], spec[k]), (entry, idrv, path, k)
    free = list(CLOUD_FREE)
    assert np.array_equal(ref["uflx"][free], ref["uflxc"][free]) and np.array_equal(ref["dflx"][free], ref["dflxc"][free])
    if entry != "nomcica icld0":
        assert np.abs(ref["dflx"] - ref["dflxc"]).max() > 1.0                   # (and the clouds of the other columns matter)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_call_launches_the_kernels_it_did(hip, oracle, entry):
    got = profiled(hip, oracle, entry)
    assert got == KERNELS[entry], (entry, "missing", sorted(KERNELS[entry] - got), "new", sorted(got - KERNELS[entry]))
