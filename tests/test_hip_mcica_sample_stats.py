"""The sample variance of the averaging McICA entries (rrtmg_lw_hip_run_mcica_samples_var, the variance outputs of
rrtmg_lw_hip_run_mcica_samples_device_view; include/rrtmg_lw_hip.h, "The sample variance"): bit for bit against nsamp calls of the
existing fused entry combined by the header's recurrence in numpy, against np.var(ddof=1), and against the CPU oracle's samples."""
import ctypes as C
import re

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.synth import make_gcm_inputs

from test_hip_mcica_samples import CASES, SEED, SENTINEL, _device_out, _inputs, _keys, _reference, _to_device  # noqa: E402
from test_mcica_sample_stats_args import VAR, recurrence  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 5e-5         # tests/test_hip_mcica_samples.py: what a sample of the library is within of the oracle's (W m-2, K d-1)
STAT = ("uflx", "dflx", "hr")


def _singles(hip, d, alpha, icld, nsamp, step):
    return [hip.rrtmg_lw_mcica_subcol_from_dict(d, SEED + s * step, 0, alpha=alpha, icld=icld) for s in range(nsamp)]


def _with_var(hip, d, alpha, icld, nsamp, step):
    return hip.rrtmg_lw_mcica_subcol_from_dict(d, SEED, 0, alpha=alpha, icld=icld, nsamp=nsamp, seedstep=step, var=True)


# ---- 1. / 2. bits, and the sense of the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_variance_equals_the_recurrence_over_single_calls(hip, oracle, case, sweeps):
    ncol, nlay, config, icld, nsamp, step = CASES[case]
    d, alpha = _inputs(oracle, ncol, nlay, config, icld)
    idrv = d["idrv"]
    singles = _singles(hip, d, alpha, icld, nsamp, step)
    got = _with_var(hip, d, alpha, icld, nsamp, step)
    plain = hip.rrtmg_lw_mcica_subcol_from_dict(d, SEED, 0, alpha=alpha, icld=icld, nsamp=nsamp, seedstep=step)
    for k in STAT:
        mean, var = recurrence([s[k] for s in singles])
        assert np.array_equal(got[k], mean), (case, k, float(np.abs(got[k] - mean).max()))
        assert np.array_equal(got[k + "_var"], var), (case, k + "_var", float(np.abs(got[k + "_var"] - var).max()))
        # the definition: not negative, and the unbiased sample variance where that is above rounding
        assert (got[k + "_var"] >= 0.0).all(), (case, k)
        ref = np.var(np.stack([s[k] for s in singles]), axis=0, ddof=1)
        big = ref > 1e-6
        rel = float((np.abs(got[k + "_var"] - ref)[big] / ref[big]).max()) if big.any() else 0.0
        print(f"case {case} {sweeps} {k}_var: max {got[k + '_var'].max():.3e}, {100 * big.mean():.0f} % above 1e-6, max rel. difference to np.var {rel:.2e}")
        assert rel <= 1e-9, (case, k, rel)
    # the remaining outputs: what the entry without variance returns
    for k in _keys(idrv):
        assert np.array_equal(got[k], plain[k]), (case, k)
    assert got["icld"] == plain["icld"]


def test_columns_without_cloud_have_no_variance(hip, oracle):
    """case a with three cloud-free columns - one in each 64-column block, the first of the ragged tail among them"""
    ncol, nlay, config, icld, nsamp, step = CASES["a"]
    d, alpha = _inputs(oracle, ncol, nlay, config, icld)
    d = dict(d)
    clear_cols = [3, 64, 129]
    cldfr = np.array(d["cldfr"], order="F")
    cldfr[clear_cols, :] = 0.0
    d["cldfr"] = cldfr
    singles = _singles(hip, d, alpha, icld, nsamp, step)
    got = _with_var(hip, d, alpha, icld, nsamp, step)
    for k in STAT:
        for s in singles[1:]:
            assert np.array_equal(s[k][clear_cols], singles[0][k][clear_cols]), k
        assert (got[k + "_var"][clear_cols] <= 1e-20).all(), (k, float(got[k + "_var"][clear_cols].max()))
    others = np.setdiff1d(np.arange(ncol), clear_cols)
    frac = float((got["uflx_var"][others].max(axis=1) > 1e-2).mean())
    print(f"cloud-free columns: max variance {max(float(got[k + '_var'][clear_cols].max()) for k in STAT):.3e}; "
          f"{100 * frac:.0f} % of the others have max uflx_var > 1e-2 (W m-2)^2")
    assert frac > 0.5


# ---- 3. the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_standard_deviation_matches_the_oracle_s_samples(hip, oracle, case):
    """Moving every sample by at most eps moves the sample standard deviation by at most 2 eps sqrt(n / (n - 1)) <= 2 sqrt(2) eps."""
    ncol, nlay, config, icld, nsamp, step = CASES[case]
    d, alpha, samples, _ = _reference(oracle, case)
    got = _with_var(hip, d, alpha, icld, nsamp, step)
    bar = 2.0 * np.sqrt(2.0) * TIGHT
    for k in STAT:
        ref = np.var(np.stack([np.asarray(s[k], dtype=np.float64) for s in samples]), axis=0, ddof=1)
        diff = float(np.abs(np.sqrt(got[k + "_var"]) - np.sqrt(ref)).max())
        print(f"case {case} {k}: max |sd_hip - sd_oracle| = {diff:.3e}, {100 * diff / bar:.1f} % of the bar {bar:.3e}; max sd {np.sqrt(ref.max()):.3e}")
        assert diff <= bar, (case, k, diff)


# ---- the C entries themselves ------------------------------------------------------------------------------------------------------------
def _host_args(hip, d, alpha, icld, seed, nsamp, step, irng, out):
    ncol, nlay = d["ncol"], d["nlay"]
    a = hip._gcm_arrays(ncol, nlay, d["play"], d["plev"], d["tlay"], d["tlev"], d["tsfc"],
                        tuple(d[k] for k in ("h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr")), d["emis"])
    cld = [hip._f(d["cldfr"], (ncol, nlay)), hip._f(d["taucld"], (16, ncol, nlay)), hip._f(d["cicewp"], (ncol, nlay)),
           hip._f(d["cliqwp"], (ncol, nlay)), hip._f(d["reice"], (ncol, nlay)), hip._f(d["reliq"], (ncol, nlay)),
           hip._f(alpha, (ncol, nlay)), hip._f(d["tauaer"], (ncol, nlay, 16))]
    icld_c, irng_c = C.c_int(icld), C.c_int(irng)
    args = [C.c_int(ncol), C.c_int(nlay), C.byref(icld_c), C.c_int(d["idrv"]), C.c_int(seed), C.c_int(nsamp), C.c_int(step), C.byref(irng_c)]
    args += [hip._p(x) for x in a] + [C.c_int(d["inflglw"]), C.c_int(d["iceflglw"]), C.c_int(d["liqflglw"])]
    args += [hip._p(x) for x in cld] + hip._out_ptrs(out, d["idrv"])
    return args, icld_c, (a, cld, irng_c)


def _raw_var_call(hip, d, alpha, icld, seed, nsamp, step, irng, out, var):
    """rrtmg_lw_hip_run_mcica_samples_var on the arrays of `out`; var: uflx_var, dflx_var, hr_var arrays, None = a null pointer"""
    args, icld_c, keep = _host_args(hip, d, alpha, icld, seed, nsamp, step, irng, out)
    null = C.cast(None, C.POINTER(C.c_double))
    rc = hip.lib().rrtmg_lw_hip_run_mcica_samples_var(*args, *[hip._p(v) if v is not None else null for v in var])
    return rc, icld_c.value


def _var_arrays(ncol, nlay, fill):
    return [np.full((ncol, nlay + 1), fill, order="F"), np.full((ncol, nlay + 1), fill, order="F"), np.full((ncol, nlay), fill, order="F")]


# ---- 4. partial outputs, nothing drawn --------------------------------------------------------------------------------------------------
def test_one_variance_alone_and_no_cloud(hip, oracle):
    ncol, nlay, config, icld, nsamp, step = CASES["a"]
    d, alpha = _inputs(oracle, ncol, nlay, config, icld)
    full = _with_var(hip, d, alpha, icld, nsamp, step)
    out = hip._out_arrays(ncol, nlay, d["idrv"])
    hr_var = np.full((ncol, nlay), SENTINEL, order="F")
    rc, _ = _raw_var_call(hip, d, alpha, icld, SEED, nsamp, step, 0, out, [None, None, hr_var])
    hip._check(rc)
    assert np.array_equal(hr_var, full["hr_var"])
    for k in _keys(d["idrv"]):
        assert np.array_equal(out[k], full[k]), k
    # icld = 0: nothing is drawn - exact zeros, written by the call, and the single call's means
    single = hip.rrtmg_lw_mcica_subcol_from_dict(d, SEED, 0, alpha=alpha, icld=0)
    out = hip._out_arrays(ncol, nlay, d["idrv"])
    var = _var_arrays(ncol, nlay, SENTINEL)
    rc, icld_out = _raw_var_call(hip, d, alpha, 0, SEED, 4, step, 0, out, var)
    hip._check(rc)
    for v in var:
        assert (v == 0.0).all()
    for k in _keys(d["idrv"]):
        assert np.array_equal(out[k], single[k]), k
    assert icld_out == single["icld"]


# ---- 5. batching ------------------------------------------------------------------------------------------------------------------------
def test_batching_is_transparent(hip, oracle):
    ncol, nlay, icld = 600, 40, 2
    d, alpha = _inputs(oracle, ncol, nlay, "cloudy", icld)
    one = _with_var(hip, d, alpha, icld, 3, 140)
    hip.set_batch(256)
    try:
        three = _with_var(hip, d, alpha, icld, 3, 140)
    finally:
        hip.set_batch(0)
    for k in _keys(d["idrv"]) + list(VAR):
        assert np.array_equal(one[k], three[k]), k
    assert np.isfinite(one["uflx_var"]).all() and one["uflx_var"].max() > 1e-2


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
def _device_call(hip, dd, al, out, var, icld, seed, nsamp, step, irng=0):
    """rrtmg_lw_hip_run_mcica_samples_device_view with the view {8, 0, 0, 0} on contiguous tensors -> return code"""
    import torch
    from rrtmg_lw_amd.api import _ArrayViewC, _FLUX_OUT, _GCM_ORDER
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    icld_c, irng_c = C.c_int(icld), C.c_int(irng)
    args = [C.byref(_ArrayViewC(8, 0, 0, 0)), C.c_int(dd["ncol"]), C.c_int(dd["nlay"]), C.byref(icld_c), C.c_int(dd["idrv"]), C.c_int(seed), C.c_int(nsamp),
            C.c_int(step), C.byref(irng_c)]
    args += [ptr(dd[k]) for k in _GCM_ORDER] + [C.c_int(dd["inflglw"]), C.c_int(dd["iceflglw"]), C.c_int(dd["liqflglw"])]
    args += [ptr(dd[k]) for k in ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq")] + [ptr(al), ptr(dd["tauaer"])]
    args += [ptr(out.get(k)) for k in _FLUX_OUT] + [ptr(v) for v in var]
    return hip.lib().rrtmg_lw_hip_run_mcica_samples_device_view(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _device_var(torch, ncol, nlay, fill):
    z = lambda *s: torch.full(s, fill, dtype=torch.float64, device="cuda:0")
    return [z(nlay + 1, ncol), z(nlay + 1, ncol), z(nlay, ncol)]


@pytest.mark.parametrize("seed,nsamp,step,irng,alias,text", [
    (SEED, 1, 140, 0, None, "uflx_var with nsamp = 1"),
    (SEED, 3, 140, 0, 0, "uflx_var aliases uflx"),
    (SEED, 3, 140, 0, 1, "dflx_var aliases dflx"),
    (SEED, 3, 140, 0, 2, "hr_var aliases hr"),
    (SEED, 0, 140, 0, None, "nsamp"),
    (SEED, 65, 140, 0, None, "nsamp = 65 exceeds RRTMG_LW_HIP_MAX_SAMPLES"),
    (SEED, 4, 0, 0, None, "seedstep"),
    (2147483647 - 100, 2, 140, 0, None, r"permuteseed \+ \(nsamp - 1\) \* seedstep"),
    (SEED, 2, 140, 1, None, "irng"),
])
def test_argument_errors_leave_the_outputs_alone(hip, oracle, seed, nsamp, step, irng, alias, text):
    import torch
    ncol, nlay, config, icld, _, _ = CASES["c"]
    d, alpha = _inputs(oracle, ncol, nlay, config, icld)
    last = lambda: hip.lib().rrtmg_lw_hip_last_error().decode()
    names = ("uflx", "dflx", "hr")
    # the host entry
    host = hip._out_arrays(ncol, nlay, d["idrv"])
    for v in host.values():
        v.fill(SENTINEL)
    var = _var_arrays(ncol, nlay, SENTINEL)
    if alias is not None:
        var[alias] = host[names[alias]]
    rc, _ = _raw_var_call(hip, d, alpha, icld, seed, nsamp, step, irng, host, var)
    assert rc == 2 and re.search(text, last()), last()
    for k, v in list(host.items()) + list(zip(VAR, var)):
        assert (v == SENTINEL).all(), k
    # the device entry
    dd = {k: _to_device(torch, v) for k, v in d.items()}
    al = _to_device(torch, np.asfortranarray(alpha))
    out = _device_out(torch, ncol, nlay, d["idrv"], SENTINEL)
    dvar = _device_var(torch, ncol, nlay, SENTINEL)
    if alias is not None:
        dvar[alias] = out[names[alias]]
    rc = _device_call(hip, dd, al, out, dvar, icld, seed, nsamp, step, irng)
    assert rc == 2 and re.search(text, last()), last()
    torch.cuda.synchronize()
    for k, v in list(out.items()) + list(zip(VAR, dvar)):
        assert bool((v == SENTINEL).all()), k


def test_physics_error_is_the_single_call_s(hip, oracle):
    import torch
    ncol, nlay, config, icld, nsamp, step = CASES["c"]
    d, alpha = _inputs(oracle, ncol, nlay, config, icld)
    d = dict(d)
    cell = np.unravel_index(np.argmax(np.asarray(d["cldfr"]) * np.asarray(d["cicewp"])), (ncol, nlay))
    reice = np.array(d["reice"], order="F")
    reice[cell] = 500.0
    d["reice"] = reice
    with pytest.raises(hip.RrtmgLwError) as single:
        hip.rrtmg_lw_mcica_subcol_from_dict(d, SEED, 0, alpha=alpha, icld=icld)
    assert "error 1:" in str(single.value) and "OUT OF BOUNDS" in str(single.value)
    with pytest.raises(hip.RrtmgLwError) as host:
        _with_var(hip, d, alpha, icld, nsamp, step)
    assert str(host.value) == str(single.value)
    dd = {k: _to_device(torch, v) for k, v in d.items()}
    al = _to_device(torch, np.asfortranarray(alpha))
    out = arrays.empty_like_form(("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + VAR, ncol, nlay, arrays.REFERENCE, device="cuda:0", fill=float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    hip.rrtmg_lw_mcica_samples_device(dd, out, SEED, nsamp, seedstep=step, alpha=al, icld=icld, stream=stream)
    with pytest.raises(hip.RrtmgLwError) as dev:
        hip.check(stream)
    assert str(dev.value) == str(single.value)
    # ... and the library goes on
    d["reice"] = make_gcm_inputs(ncol, nlay, config, col0=31)["reice"]
    assert np.isfinite(_with_var(hip, d, alpha, icld, 2, 140)["uflx_var"]).all()
