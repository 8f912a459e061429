"""rrtmg_lw_hip_run_mcica_samples_device_view and rrtmg_lw_hip_get_alpha_device_view (include/rrtmg_lw_hip.h): the mean over several
sub-column samples, its variances and get_alpha on device arrays in the caller's own form and width.  The method of
tests/test_hip_device_views.py - array_equal, no tolerance: the results equal what the plain entries return on contiguous float64
reference-form copies of the call's columns, put into the form; output fields are prefilled with a NaN bit pattern and nothing outside
the call's columns is written; input fields hold NaN outside the call's columns."""
import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import REFERENCE, ArrayForm

from test_hip_device_views import FLUX, _check_outputs, _dev, _embed_inputs, _host, _int, _output_fields, _stream, fid  # noqa: E402
from test_hip_mcica_samples import CASES, SEED, _inputs  # noqa: E402
from test_mcica_sample_stats_args import VAR  # noqa: E402

pytestmark = pytest.mark.gpu

R4, R8TOP, R4LFTOP = ArrayForm(4, 0, 0), ArrayForm(8, 0, 1), ArrayForm(4, 1, 1)
PAD, C0 = 5, 4            # fields ncol + 5 wide, the call's columns from column 4
SENTINEL = -777.25


def _names(idrv):
    return FLUX if idrv == 1 else FLUX[:6]


_REF = {}


def _plain(hip, oracle, case, form):
    """Once per (case, form): the inputs of the case in `form` (numpy, the call's columns and nothing else; alpha among them) and what
    the PLAIN entries return on those inputs widened to the float64 reference form, put into the form: the means and the clear-sky
    outputs of rrtmg_lw_hip_run_mcica_samples_device, the variances of the new entry with the view {8, 0, 0, 0} - whose other outputs
    must be the plain entry's.  Shared by the tests and left unchanged."""
    form = ArrayForm(*form)
    key = (case, tuple(form))
    if key in _REF:
        return _REF[key]
    ncol, nlay, config, icld, nsamp, step = CASES[case]
    d, alpha = _inputs(oracle, ncol, nlay, config, icld)
    x = arrays.from_reference(dict(d, alpha=np.asfortranarray(alpha)), form)
    wd = _dev(arrays.to_reference(x, form))
    al = wd["alpha"] if icld in (4, 5) else None
    names = _names(d["idrv"])
    s = _stream()
    old = arrays.empty_like_form(names, ncol, nlay, REFERENCE, device="cuda:0", fill=float("nan"))
    icld_old = hip.rrtmg_lw_mcica_subcol_device(wd, old, SEED, 0, alpha=al, icld=icld, stream=s, nsamp=nsamp, seedstep=step)
    new = arrays.empty_like_form(names + VAR, ncol, nlay, REFERENCE, device="cuda:0", fill=float("nan"))
    icld_new = hip.rrtmg_lw_mcica_samples_device(wd, new, SEED, nsamp, seedstep=step, alpha=al, icld=icld, stream=s)
    hip.check(s)
    old, new = _host(old), _host(new)
    assert icld_old == icld_new
    for k in names:
        assert np.isfinite(old[k]).all() and np.array_equal(new[k], old[k]), (case, k)
    for k in VAR:
        assert np.isfinite(new[k]).all() and (new[k] >= 0).all() and new[k].max() > 0, (case, k)
    want = arrays.from_reference(new, form)
    for v in want.values():
        v.setflags(write=False)
    _REF[key] = (x, want, icld_new)
    return _REF[key]


def _run(hip, oracle, case, form, ld, c0, var=VAR):
    """the new entry on views of fields ld wide (0: contiguous tensors of the form) -> (fields, views)"""
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    ncol, nlay, config, icld, nsamp, step = CASES[case]
    x, want, icld_ref = _plain(hip, oracle, case, form)
    xin = _embed_inputs(x, form, ld or ncol, c0, _GCM_ORDER + _CLD_ORDER + ("alpha",))
    d = dict(x, **xin)
    names = _names(x["idrv"]) + tuple(var)
    fields, views = _output_fields(names, ncol, nlay, form, ld or ncol, c0)
    s = _stream()
    icld_out = hip.rrtmg_lw_mcica_samples_device(d, views, SEED, nsamp, seedstep=step, alpha=d["alpha"] if icld in (4, 5) else None, icld=icld,
                                                 stream=s, form=None if form == REFERENCE else form, ld=ld)
    hip.check(s)
    assert icld_out == icld_ref
    _check_outputs(fields, views, want, names, form, ncol, c0)
    return fields, views


# ---- 7. in place ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b"])
def test_samples_in_place_in_a_wider_field(hip, oracle, case):
    ncol = CASES[case][0]
    fields, views = _run(hip, oracle, case, REFERENCE, ncol + PAD, C0)
    first = {k: v.clone() for k, v in fields.items()}
    # again, into fresh output fields: they are written, and the first set is not touched
    _run(hip, oracle, case, REFERENCE, ncol + PAD, C0)
    for k in fields:
        assert bool((_int(fields[k], 8) == _int(first[k], 8)).all()), k


@pytest.mark.parametrize("case", ["a", "b"])
def test_the_mean_alone(hip, oracle, case):
    """all three variance pointers null: the mean in the host's own form"""
    ncol = CASES[case][0]
    _run(hip, oracle, case, REFERENCE, ncol + PAD, C0, var=())
    _run(hip, oracle, case, R4, ncol + PAD, C0, var=())


# ---- 8. forms ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def batch64(hip):
    hip.set_batch(64)
    try:
        yield
    finally:
        hip.set_batch(0)


@pytest.mark.parametrize("form,wide", [(R4, True), (R8TOP, True), (R4LFTOP, False)], ids=lambda v: fid(v) if isinstance(v, tuple) else "")
def test_samples_in_a_converting_form(hip, oracle, form, wide, batch64):
    """case a, 130 columns in staged batches of 64, 64 and 2"""
    ncol = CASES["a"][0]
    _run(hip, oracle, "a", form, ncol + PAD if wide else 0, C0 if wide else 0)


@pytest.mark.parametrize("form,wide", [(R4, True), (R8TOP, True), (R4LFTOP, False)], ids=lambda v: fid(v) if isinstance(v, tuple) else "")
def test_samples_in_a_converting_form_with_alpha_and_ddt(hip, oracle, form, wide):
    """case b: idrv = 1, exponential-random overlap - alpha is staged with the batch"""
    ncol = CASES["b"][0]
    _run(hip, oracle, "b", form, ncol + PAD if wide else 0, C0 if wide else 0)


# ---- 9. get_alpha -----------------------------------------------------------------------------------------------------------------------
ALPHA_NCOL, ALPHA_NLAY, DECORR = 130, 40, 2500.0


def _alpha_inputs(oracle, icld):
    d, _ = _inputs(oracle, ALPHA_NCOL, ALPHA_NLAY, "cloudy", icld)
    rng = np.random.default_rng(3)                      # (dz and lat as _inputs draws them)
    dz, lat = rng.uniform(100, 1500, (ALPHA_NCOL, ALPHA_NLAY)), rng.uniform(-90, 90, ALPHA_NCOL)
    return d, {"ncol": ALPHA_NCOL, "nlay": ALPHA_NLAY, "dz": np.asfortranarray(dz), "lat": lat, "cldfr": np.asfortranarray(d["cldfr"])}


def _alpha_view(hip, g, form, ld, c0, icld, idcor, juldat):
    """get_alpha_device on views of fields ld wide that hold NaN elsewhere -> (the alpha field, its view)"""
    ncol, nlay = g["ncol"], g["nlay"]
    xin = _embed_inputs(g, form, ld or ncol, c0, ("dz", "lat", "cldfr"))
    fields, views = _output_fields(("alpha",), ncol, nlay, form, ld or ncol, c0)
    s = _stream()
    hip.get_alpha_device(dict(g, **xin), views["alpha"], icld, idcor, DECORR, juldat, stream=s, form=None if form == REFERENCE else form, ld=ld)
    hip.check(s)
    return fields, views


@pytest.mark.parametrize("icld,idcor,juldat", [(4, 0, 100), (5, 0, 100), (5, 1, 100), (5, 1, 250), (4, 1, 40)])
def test_alpha_on_the_device(hip, oracle, icld, idcor, juldat):
    ncol, nlay = ALPHA_NCOL, ALPHA_NLAY
    _, g = _alpha_inputs(oracle, icld)
    host = hip.get_alpha(ncol, nlay, icld, idcor, DECORR, g["dz"], g["lat"], juldat, g["cldfr"])
    ref = oracle.get_alpha(ncol, nlay, icld, idcor, DECORR, g["dz"], g["lat"], juldat, g["cldfr"])
    assert host.max() > 0.1
    # the plain view on contiguous tensors: the host entry's bits
    fields, views = _alpha_view(hip, g, REFERENCE, 0, 0, icld, idcor, juldat)
    got = views["alpha"].cpu().numpy()
    assert np.array_equal(got, host)
    assert np.abs(got - ref).max() <= 1e-15
    # in place in a wider field, and the converting forms: the plain result on the widened inputs, rounded; nothing else is written
    for form, wide in ((REFERENCE, True), (R4, True), (R8TOP, True), (R4LFTOP, False)):
        x = arrays.from_reference(g, form)
        w = arrays.to_reference(x, form)
        want = arrays.from_reference({"alpha": hip.get_alpha(ncol, nlay, icld, idcor, DECORR, w["dz"], w["lat"], juldat, w["cldfr"])}, form)
        ld, c0 = (ncol + PAD, C0) if wide else (0, 0)
        fields, views = _alpha_view(hip, x, form, ld, c0, icld, idcor, juldat)
        _check_outputs(fields, views, want, ("alpha",), form, ncol, c0)


def test_alpha_is_left_alone_without_an_exponential_overlap(hip, oracle):
    import torch
    _, g = _alpha_inputs(oracle, 2)
    gd = _dev(g)
    alpha = torch.full((ALPHA_NLAY, ALPHA_NCOL), SENTINEL, dtype=torch.float64, device="cuda:0").permute(1, 0)
    s = _stream()
    hip.get_alpha_device(gd, alpha, 2, 1, DECORR, 100, stream=s)
    hip.check(s)
    assert bool((alpha == SENTINEL).all())


def test_device_alpha_feeds_the_samples_entry(hip, oracle):
    """case b's shape and overlap: alpha made on the device, in a float32 top-first field, goes straight into the averaging entry"""
    ncol, nlay, config, icld, nsamp, step = CASES["b"]
    form = ArrayForm(4, 0, 1)
    d, _ = _inputs(oracle, ncol, nlay, config, icld)
    rng = np.random.default_rng(3)
    dz, lat = rng.uniform(100, 1500, (ncol, nlay)), rng.uniform(-90, 90, ncol)
    x = arrays.from_reference(dict(d, dz=np.asfortranarray(dz), lat=lat), form)
    w = arrays.to_reference(x, form)
    # the host's alpha for the widened inputs, rounded as the form stores it
    x_host = dict(x, **arrays.from_reference({"alpha": hip.get_alpha(ncol, nlay, icld, 1, DECORR, w["dz"], w["lat"], 100, w["cldfr"])}, form))
    xd = _dev(x)
    names = _names(d["idrv"]) + VAR
    s = _stream()
    alpha = arrays.empty_like_form(("alpha",), ncol, nlay, form, device="cuda:0", fill=float("nan"))["alpha"]
    hip.get_alpha_device(xd, alpha, icld, 1, DECORR, 100, stream=s, form=form)
    out = arrays.empty_like_form(names, ncol, nlay, form, device="cuda:0", fill=float("nan"))
    hip.rrtmg_lw_mcica_samples_device(xd, out, SEED, nsamp, seedstep=step, alpha=alpha, icld=icld, stream=s, form=form)
    want = arrays.empty_like_form(names, ncol, nlay, form, device="cuda:0", fill=float("nan"))
    xh = _dev(x_host)
    hip.rrtmg_lw_mcica_samples_device(xh, want, SEED, nsamp, seedstep=step, alpha=xh["alpha"], icld=icld, stream=s, form=form)
    hip.check(s)
    assert bool((_int(alpha, 4) == _int(xh["alpha"], 4)).all())
    for k in names:
        assert bool(out[k].isfinite().all()) and bool((_int(out[k], 4) == _int(want[k], 4)).all()), k
