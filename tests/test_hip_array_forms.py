"""The *_as device entries (include/rrtmg_lw_hip.h, rrtmg_lw_hip_array_form): device arrays in float32 / (column, level) C order / top
first, converted on the device around the solver.  The defining property, checked here with array_equal and no tolerance: for every form
the results equal what the plain entry gives on the same values brought into the reference form - float32 inputs widened, float32
outputs rounded.  The tests build their arrays with rrtmg_lw_amd.arrays (written from the header's table, tested on the CPU in
tests/test_array_forms.py), never with the library.

Shapes: 333 columns x 33 layers (ragged 64-column tiles, an odd layer count, ragged 64-value tiles in every array), 200 x 70 (more than
64 layers: two tiles along the vertical), set_batch(128) around some cases (several batches, a ragged last one)."""
import ctypes as C

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import ALL_FORMS, REFERENCE, ArrayForm
from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

FLUX = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
OPTICS = ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt")
EARG, EPHYSICS = 2, 1


def _dev(a):
    """numpy array or dict of them -> CUDA tensors that lie in memory exactly as the arrays do"""
    import torch
    if isinstance(a, dict):
        return {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    t = torch.from_numpy(a).to("cuda:0")
    assert tuple(s * t.element_size() for s in t.stride()) == a.strides
    return t


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


def _inputs(case):
    """the reference-form inputs of a named case (numpy, float64)"""
    if case == "aer_idrv":                     # clouds, aerosol, idrv = 1, inflglw / iceflglw / liqflglw = 2 / 3 / 1
        d = make_gcm_inputs(333, 33, "aer_idrv", col0=17)
        assert (d["idrv"], d["icld"], d["inflglw"], d["iceflglw"], d["liqflglw"]) == (1, 2, 2, 3, 1)
    elif case == "tall":                       # more than 64 layers
        d = make_gcm_inputs(200, 70, "aer_idrv", col0=5)
    elif case == "inflag0":                    # taucld used band by band: every band another value in the cloudy cells
        d = make_gcm_inputs(333, 33, "cloudy", col0=3)
        b = (0.3 + 0.45 * np.arange(16))[:, None, None]
        cell = 1.0 + (np.arange(333)[:, None] % 7) * 0.25 + (np.arange(33)[None, :] % 5) * 0.125
        d["taucld"] = np.asfortranarray(b * (np.array(d["cldfr"]) > 0)[None] * cell[None])
        d["inflglw"], d["iceflglw"], d["liqflglw"] = 0, 0, 0
    elif case == "mcica":
        d = make_gcm_inputs(333, 33, "cloudy", col0=40)
        u = np.random.default_rng(11).random((333, 33))
        d["alpha"] = np.asfortranarray(0.1 + 0.8 * u)
    elif case == "other":                      # what a later plain call runs on
        d = make_gcm_inputs(150, 33, "cloudy", col0=900)
    else:
        raise KeyError(case)
    return d


_REF = {}


def _reference(hip, case, real_bytes, kind="nomcica", **kw):
    """Once per (case, precision, call): the inputs as the form's precision leaves them, widened (float64 reference form), and the plain
    entry's results on them.  Shared by the tests and left unchanged."""
    import torch
    key = (case, real_bytes, kind, tuple(sorted(kw.items())), hip.gpoints())
    if key not in _REF:
        d = _inputs(case)
        wide = arrays.to_reference(arrays.from_reference(d, ArrayForm(real_bytes, 0, 0)), ArrayForm(real_bytes, 0, 0))
        if real_bytes == 8:
            assert all(np.array_equal(wide[k], d[k]) for k in d if isinstance(d[k], np.ndarray))
        dd = _dev(wide)
        ncol, nlay = d["ncol"], d["nlay"]
        s = torch.cuda.current_stream().cuda_stream
        if kind == "optics":
            out = arrays.empty_like_form(OPTICS, ncol, nlay, REFERENCE, hip.gpoints(), device="cuda:0", fill=float("nan"))
            hip.gas_optics_device(dd, out, stream=s, idrv=1)
            icld = None
        else:
            out = arrays.empty_like_form(FLUX, ncol, nlay, REFERENCE, device="cuda:0", fill=float("nan"))
            if kind == "nomcica":
                icld = hip.rrtmg_lw_device(dd, out, stream=s, **kw)
            else:
                alpha = dd.get("alpha") if kw["icld"] in (4, 5) else None
                icld = hip.rrtmg_lw_mcica_subcol_device(dd, out, kw["seed"], kw["irng"], alpha=alpha, icld=kw["icld"], stream=s)
        hip.check(s)
        res = _host(out)
        for v in res.values():
            v.setflags(write=False)
        _REF[key] = (wide, res, icld)
    return _REF[key]


def _compare(got, ref_out, form, names, ncol, nlay, ng=140):
    """every output, in the caller's form, equals the plain entry's result brought into that form (float32: rounded) - and the other
    way round through to_reference"""
    want = arrays.from_reference({k: ref_out[k] for k in names}, form)
    back = arrays.to_reference(got, form)
    dt = np.float64 if form.real_bytes == 8 else np.float32
    for k in names:
        assert got[k].dtype == dt and got[k].shape == arrays.form_shape(k, ncol, nlay, form, ng), k
        assert np.isfinite(got[k]).all(), k
        assert np.array_equal(got[k], want[k]), (k, tuple(form), float(np.abs(got[k].astype(np.float64) - want[k]).max()))
        assert np.array_equal(back[k], np.asarray(ref_out[k]).astype(dt).astype(np.float64)), k


def _run_as(hip, wide, form, idrv=None, icld=None, names=FLUX):
    import torch
    ncol, nlay = wide["ncol"], wide["nlay"]
    x = _dev(arrays.from_reference(wide, form))
    out = arrays.empty_like_form(names, ncol, nlay, form, device="cuda:0", fill=float("nan"))
    s = torch.cuda.current_stream().cuda_stream
    kw = {} if icld is None else {"icld": icld}
    if idrv is not None:
        kw["idrv"] = idrv
    ic = hip.rrtmg_lw_device(x, out, stream=s, form=form, **kw)
    hip.check(s)
    return _host(out), ic


@pytest.fixture()
def batch128(hip):
    hip.set_batch(128)
    try:
        yield
    finally:
        hip.set_batch(0)


# ---- 1. rrtmg_lw_hip_run_nomcica_device_as --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL_FORMS, ids=lambda f: "r%d_lf%d_top%d" % tuple(f))
def test_nomcica_every_form_equals_the_plain_entry(hip, form):
    wide, ref, icld = _reference(hip, "aer_idrv", form.real_bytes)
    got, ic = _run_as(hip, wide, form)
    assert ic == icld == 2
    _compare(got, ref, form, FLUX, 333, 33)


@pytest.mark.parametrize("form", [ArrayForm(4, 1, 1), ArrayForm(8, 0, 1), ArrayForm(8, 1, 0)], ids=str)
def test_nomcica_more_than_64_layers_in_several_batches(hip, batch128, form):
    """200 columns x 70 layers with 128 columns per batch: two batches, the second 72 columns wide; two tiles along the vertical"""
    assert hip.effective_batch(70) == 128
    wide, ref, _ = _reference(hip, "tall", form.real_bytes)
    got, _ = _run_as(hip, wide, form)
    _compare(got, ref, form, FLUX, 200, 70)


@pytest.mark.parametrize("form", [ArrayForm(4, 1, 1), ArrayForm(8, 0, 1), ArrayForm(4, 0, 0)], ids=str)
def test_nomcica_taucld_band_by_band(hip, form):
    """inflglw = 0: the solver reads all sixteen bands of taucld (no band sum is staged)"""
    wide, ref, _ = _reference(hip, "inflag0", form.real_bytes)
    assert len(np.unique(np.array(wide["taucld"])[:, np.array(wide["cldfr"]) > 0].T.round(3), axis=1)) > 1
    assert np.abs(ref["uflx"] - ref["uflxc"]).max() > 0.0            # the clouds are seen
    got, _ = _run_as(hip, wide, form)
    names = FLUX[:6]                                                 # idrv = 0: no d/dT outputs
    _compare(got, ref, form, names, 333, 33)
    assert all(np.isnan(got[k]).all() for k in FLUX[6:])             # ... and they are left untouched


def test_nomcica_several_batches_with_band_sum_and_ragged_last(hip, batch128):
    """333 columns in batches of 128, 128 and 77 with the band sum of taucld staged (inflglw = 2)"""
    form = ArrayForm(4, 1, 1)
    wide, ref, _ = _reference(hip, "aer_idrv", 4)
    got, _ = _run_as(hip, wide, form)
    _compare(got, ref, form, FLUX, 333, 33)


def test_nomcica_icld_zero_and_out_of_range(hip):
    form = ArrayForm(4, 1, 1)
    wide, ref, icld = _reference(hip, "aer_idrv", 4, icld=0)
    got, ic = _run_as(hip, wide, form, icld=0)
    assert ic == icld == 0
    _compare(got, ref, form, FLUX, 333, 33)
    assert np.array_equal(ref["uflx"], ref["uflxc"])
    # an icld outside [0, 3] comes back as 2 and is solved as such
    wide, ref2, icld = _reference(hip, "aer_idrv", 4, icld=7)
    got, ic = _run_as(hip, wide, form, icld=7)
    assert ic == icld == 2
    _compare(got, ref2, form, FLUX, 333, 33)
    assert np.array_equal(ref2["uflx"], _reference(hip, "aer_idrv", 4)[1]["uflx"])


# ---- 2. rrtmg_lw_hip_run_mcica_subcol_device_as ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,irng,icld,batch", [(ArrayForm(4, 1, 1), 0, 2, 0), (ArrayForm(4, 1, 1), 1, 5, 128),
                                                   (ArrayForm(8, 1, 0), 1, 2, 0), (ArrayForm(8, 1, 0), 0, 5, 128)], ids=str)
def test_fused_mcica_equals_the_plain_fused_entry(hip, form, irng, icld, batch):
    """both generators; maximum-random overlap and exponential-random with alpha; with batch = 128 the 333 columns are three batches
    while the generator - the Mersenne Twister's one stream over all columns - runs over the whole call"""
    import torch
    wide, ref, ic_ref = _reference(hip, "mcica", form.real_bytes, kind="mcica", seed=7, irng=irng, icld=icld)
    assert np.abs(ref["uflx"] - ref["uflxc"]).max() > 0.0
    names = FLUX[:6]
    hip.set_batch(batch)
    try:
        x = _dev(arrays.from_reference(wide, form))
        alpha = x.pop("alpha")
        out = arrays.empty_like_form(names, 333, 33, form, device="cuda:0", fill=float("nan"))
        s = torch.cuda.current_stream().cuda_stream
        ic = hip.rrtmg_lw_mcica_subcol_device(x, out, 7, irng, alpha=alpha if icld == 5 else None, icld=icld, stream=s, form=form)
        hip.check(s)
    finally:
        hip.set_batch(0)
    assert ic == ic_ref == 2
    _compare(_host(out), ref, form, names, 333, 33)


# ---- 3. rrtmg_lw_hip_gas_optics_device_as ------------------------------------------------------------------------------------------------
def _run_optics_as(hip, wide, form, idrv, out):
    import torch
    x = _dev(arrays.from_reference({k: v for k, v in wide.items() if k not in ("alpha",)}, form))
    s = torch.cuda.current_stream().cuda_stream
    hip.gas_optics_device(x, out, stream=s, idrv=idrv, form=form)
    hip.check(s)


@pytest.mark.parametrize("form", [ArrayForm(4, 1, 1), ArrayForm(8, 1, 0), ArrayForm(4, 0, 0)], ids=str)
def test_gas_optics_equals_the_plain_entry(hip, form):
    wide, ref, _ = _reference(hip, "aer_idrv", form.real_bytes, kind="optics")
    out = arrays.empty_like_form(OPTICS, 333, 33, form, hip.gpoints(), device="cuda:0", fill=float("nan"))
    _run_optics_as(hip, wide, form, 1, out)
    _compare(_host(out), ref, form, OPTICS, 333, 33, hip.gpoints())


def test_gas_optics_several_batches(hip, batch128):
    form = ArrayForm(4, 1, 1)
    wide, ref, _ = _reference(hip, "tall", 4, kind="optics")
    out = arrays.empty_like_form(OPTICS, 200, 70, form, hip.gpoints(), device="cuda:0", fill=float("nan"))
    _run_optics_as(hip, wide, form, 1, out)
    _compare(_host(out), ref, form, OPTICS, 200, 70, hip.gpoints())


def test_gas_optics_optional_outputs(hip):
    """the Planck outputs NULL: not formed; dplankbnd_dt with idrv = 0: left untouched (a sentinel stays)"""
    form = ArrayForm(4, 1, 1)
    wide, ref, _ = _reference(hip, "aer_idrv", 4, kind="optics")
    out = arrays.empty_like_form(("taug", "fracs", "dplankbnd_dt"), 333, 33, form, hip.gpoints(), device="cuda:0", fill=-777.0)
    out.update(planklay=None, planklev=None, plankbnd=None)
    _run_optics_as(hip, wide, form, 0, out)
    got = _host(out)
    _compare(got, ref, form, ("taug", "fracs"), 333, 33, hip.gpoints())
    assert (got["dplankbnd_dt"] == -777.0).all()


@pytest.fixture()
def hip256(hip):
    """The session's 140-point library stays loaded; the 256-point one is selected for the test and deselected afterwards."""
    hip.select_gpoints(256)
    try:
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        yield hip
        hip.finalize(selected_only=True)
    finally:
        hip.select_gpoints(140)


def test_gas_optics_256_g_points(hip256):
    assert hip256.gpoints() == 256
    form = ArrayForm(4, 1, 1)
    wide, ref, _ = _reference(hip256, "aer_idrv", 4, kind="optics")
    assert ref["taug"].shape == (333, 33, 256)
    out = arrays.empty_like_form(OPTICS, 333, 33, form, 256, device="cuda:0", fill=float("nan"))
    _run_optics_as(hip256, wide, form, 1, out)
    _compare(_host(out), ref, form, OPTICS, 333, 33, 256)


# ---- 4. the plain form ---------------------------------------------------------------------------------------------------------------------
def test_reference_form_forwards_to_the_plain_entry(hip):
    wide, ref, _ = _reference(hip, "aer_idrv", 8)
    got, ic = _run_as(hip, wide, REFERENCE)
    assert ic == 2
    _compare(got, ref, REFERENCE, FLUX, 333, 33)
    wide, ref, _ = _reference(hip, "aer_idrv", 8, kind="optics")
    out = arrays.empty_like_form(OPTICS, 333, 33, REFERENCE, hip.gpoints(), device="cuda:0", fill=float("nan"))
    _run_optics_as(hip, wide, REFERENCE, 1, out)
    _compare(_host(out), ref, REFERENCE, OPTICS, 333, 33, hip.gpoints())


# ---- 5. arguments --------------------------------------------------------------------------------------------------------------------------
class _Form(C.Structure):
    _fields_ = [("real_bytes", C.c_int), ("layer_fastest", C.c_int), ("top_first", C.c_int)]


def _raw_args(hip, x, out, drop=None):
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    p = lambda k, src: C.c_void_p(0 if k == drop else src[k].data_ptr())
    icld = C.c_int(2)
    a = [C.c_int(x["ncol"]), C.c_int(x["nlay"]), C.byref(icld), C.c_int(1)] + [p(k, x) for k in _GCM_ORDER]
    a += [C.c_int(2), C.c_int(3), C.c_int(1)] + [p(k, x) for k in _CLD_ORDER] + [p(k, out) for k in FLUX] + [C.c_void_p(0)]
    return a


def test_bad_arguments_are_earg_with_a_message(hip):
    lib = hip.lib()
    form = ArrayForm(4, 1, 1)
    wide, _, _ = _reference(hip, "aer_idrv", 4)
    x = _dev(arrays.from_reference(wide, form))
    out = arrays.empty_like_form(FLUX, 333, 33, form, device="cuda:0", fill=-1.0)
    msg = lambda: lib.rrtmg_lw_hip_last_error().decode()
    fn = lib.rrtmg_lw_hip_run_nomcica_device_as
    assert fn(None, *_raw_args(hip, x, out)) == EARG and "form" in msg()
    assert fn(C.byref(_Form(2, 1, 1)), *_raw_args(hip, x, out)) == EARG and "real_bytes" in msg()
    assert fn(C.byref(_Form(4, 2, 1)), *_raw_args(hip, x, out)) == EARG and "layer_fastest" in msg()
    assert fn(C.byref(_Form(4, 1, 2)), *_raw_args(hip, x, out)) == EARG and "top_first" in msg()
    assert fn(C.byref(_Form(4, 1, 1)), *_raw_args(hip, x, out, drop="tlev")) == EARG and "null input" in msg()
    assert fn(C.byref(_Form(4, 1, 1)), *_raw_args(hip, x, out, drop="reice")) == EARG and "null input" in msg()
    assert fn(C.byref(_Form(4, 1, 1)), *_raw_args(hip, x, out, drop="hrc")) == EARG and "null output" in msg()
    assert fn(C.byref(_Form(4, 1, 1)), *_raw_args(hip, x, out, drop="duflx_dt")) == EARG and "idrv=1" in msg()
    # the other two entries check the form the same way
    g = lib.rrtmg_lw_hip_gas_optics_device_as
    from rrtmg_lw_amd.api import _GCM_ORDER
    oa = [C.c_int(333), C.c_int(33), C.c_int(0)] + [C.c_void_p(x[k].data_ptr()) for k in _GCM_ORDER] + [C.c_void_p(0)] * 7
    assert g(None, *oa) == EARG and "form" in msg()
    assert g(C.byref(_Form(3, 0, 0)), *oa) == EARG and "real_bytes" in msg()
    assert g(C.byref(_Form(4, 1, 1)), *oa) == EARG and "taug and fracs" in msg()
    m = lib.rrtmg_lw_hip_run_mcica_subcol_device_as
    ma = _raw_args(hip, x, out)
    irng = C.c_int(0)
    ma = ma[:4] + [C.c_int(1), C.byref(irng)] + ma[4:29] + [C.c_void_p(0)] + ma[29:]        # permuteseed, irng; alpha in front of tauaer
    assert m(None, *ma) == EARG and "form" in msg()
    assert m(C.byref(_Form(8, 1, -1)), *ma) == EARG and "top_first" in msg()
    assert all((v == -1.0).all() for v in _host(out).values())          # nothing was written


def test_a_particle_size_out_of_bounds_is_reported_by_check(hip):
    """one column's ice effective size outside the parameterisation's range: an error return of check(stream) with the reference's text,
    as from the plain entry"""
    import torch
    d = dict(_inputs("aer_idrv"))
    cld = np.argwhere(np.array(d["cldfr"]) > 0.1)
    i, k = cld[len(cld) // 2]
    reice = np.array(d["reice"])
    reice[i, k] = 500.0
    d["reice"] = np.asfortranarray(reice)
    s = torch.cuda.current_stream().cuda_stream
    texts = []
    for form in (REFERENCE, ArrayForm(4, 1, 1)):
        x = _dev(arrays.from_reference(d, form))
        out = arrays.empty_like_form(FLUX, 333, 33, form, device="cuda:0")
        if form.is_reference:
            hip.rrtmg_lw_device(x, out, stream=s)
        else:
            hip.rrtmg_lw_device(x, out, stream=s, form=form)
        with pytest.raises(hip.RrtmgLwError, match="error %d" % EPHYSICS) as e:
            hip.check(s)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "ICE" in texts[0]
    hip.check(s)                                     # the error word is cleared: the next call starts clean


# ---- 6. what an adapted call leaves behind -------------------------------------------------------------------------------------------------
def _staged_bytes(names, nb, nlay, ng=140):
    return 8 * sum(arrays.form_size(k, nb, nlay, REFERENCE, ng) for k in names)


@pytest.mark.parametrize("kind", ["nomcica", "mcica"])
def test_staging_is_bounded_and_leaves_the_plain_entry_alone(hip, kind):
    import torch
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)          # a re-initialisation: staging of earlier tests is gone
    s = torch.cuda.current_stream().cuda_stream
    form = ArrayForm(4, 1, 1)
    other = _dev(_inputs("other"))
    o_before = arrays.empty_like_form(FLUX[:6], 150, 33, REFERENCE, device="cuda:0", fill=float("nan"))
    hip.rrtmg_lw_device(other, o_before, stream=s)
    kw = dict(kind="mcica", seed=3, irng=0, icld=5) if kind == "mcica" else {}
    case = "mcica" if kind == "mcica" else "aer_idrv"
    wide, ref, _ = _reference(hip, case, 4, **kw)
    # the plain call of this shape, so that the solver's workspace (and the generator's buffers) stand before the adapted one
    dd = _dev(wide)
    op = arrays.empty_like_form(FLUX, 333, 33, REFERENCE, device="cuda:0")
    if kind == "mcica":
        hip.rrtmg_lw_mcica_subcol_device(dd, op, 3, 0, alpha=dd["alpha"], icld=5, stream=s)
    else:
        hip.rrtmg_lw_device(dd, op, stream=s)
    hip.check(s)
    ws0 = hip.workspace_bytes()
    names = FLUX[:6] if kind == "mcica" else FLUX
    x = _dev(arrays.from_reference(wide, form))
    out = arrays.empty_like_form(names, 333, 33, form, device="cuda:0", fill=float("nan"))
    if kind == "mcica":
        alpha = x.pop("alpha")
        hip.rrtmg_lw_mcica_subcol_device(x, out, 3, 0, alpha=alpha, icld=5, stream=s, form=form)
    else:
        hip.rrtmg_lw_device(x, out, stream=s, form=form)
    hip.check(s)
    ws1 = hip.workspace_bytes()
    nb = min(333, hip.effective_batch(33))
    bound = _staged_bytes(_GCM_ORDER + _CLD_ORDER + names, nb, 33)
    if kind == "mcica":
        bound += 3 * 333 * 33 * 8                           # play, cldfr, alpha of the whole call for the generator
    assert 0 < ws1 - ws0 <= bound, (ws1 - ws0, bound)
    _compare(_host(out), ref, form, names, 333, 33)
    # a second adapted call of the same shape allocates nothing
    if kind == "nomcica":
        hip.rrtmg_lw_device(x, out, stream=s, form=form)
        hip.check(s)
        assert hip.workspace_bytes() == ws1
    # the plain entry on other arrays: its usual result
    o_after = arrays.empty_like_form(FLUX[:6], 150, 33, REFERENCE, device="cuda:0", fill=float("nan"))
    hip.rrtmg_lw_device(other, o_after, stream=s)
    hip.check(s)
    a, b = _host(o_before), _host(o_after)
    for k in FLUX[:6]:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    hip.finalize()
    assert hip.workspace_bytes() == 0
    hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)          # (the session's fixture finalises again at the end)
