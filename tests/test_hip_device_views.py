"""The *_view device entries (include/rrtmg_lw_hip.h, rrtmg_lw_hip_array_view): the call's columns inside column-fastest device arrays
`ld` columns wide, every pointer at the call's first column.  The method of tests/test_hip_array_forms.py - array_equal, no tolerance:

  * the results equal what the EXISTING entry of the same form returns on contiguous copies of the call's columns (the plain / spectral
    device entry for {8,0,0}, the *_as entry for a converting form; spectral outputs of a converting form: the spectral device entry's,
    brought into the form on the host with rrtmg_lw_amd.arrays), bit for bit;
  * every output field is prefilled with a fixed NaN bit pattern and compared as integers afterwards: nothing outside the call's
    columns - the padding of each row, the other columns of the field - is written;
  * every input field holds NaN outside the call's columns: their contents never reach a result.

Shapes: 333 columns x 33 layers in fields ld = 401 wide from column c0 = 37 (stride and offset odd: float64 rows 8- but not 16-byte
aligned, float32 rows 4- but not 8-byte aligned; ragged 64- and 256-column tiles), the same with set_batch(128) (three batches, a ragged
last one), 200 x 70 with ld = 201, c0 = 0 (more than 64 layers), ld = ncol (the plain call)."""
import ctypes as C

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import REFERENCE, ArrayForm
from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

FLUX = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
SPEC = ("uflxs", "dflxs", "uflxcs", "dflxcs")
OPTICS = ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt")
ADJ_IN = ("plev", "dtsfc", "uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")
ADJ_OUT = ("uflx_adj", "hr_adj", "uflxc_adj", "hrc_adj")
EARG = 2
R8, R4, R8TOP = REFERENCE, ArrayForm(4, 0, 0), ArrayForm(8, 0, 1)
FORMS = [R8, R4, R8TOP]
fid = lambda f: "r%d_lf%d_top%d" % tuple(f)
PATTERN = {8: 0x7FF8DEAD0000BEEF, 4: 0x7FC0BEEF}          # quiet NaNs with a payload no computation produces
LD, C0 = 401, 37


def _dev(a):
    import torch
    if isinstance(a, dict):
        return {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    t = torch.from_numpy(a).to("cuda:0")
    assert tuple(s * t.element_size() for s in t.stride()) == a.strides
    return t


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


def _inputs(case):
    if case == "aer_idrv":                     # clouds, aerosol, idrv = 1, inflglw / iceflglw / liqflglw = 2 / 3 / 1
        d = make_gcm_inputs(333, 33, "aer_idrv", col0=17)
    elif case == "tall":                       # more than 64 layers
        d = make_gcm_inputs(200, 70, "aer_idrv", col0=5)
    elif case == "inflag0":                    # the 16-wide taucld, read band by band
        d = make_gcm_inputs(333, 33, "cloudy", col0=3)
        b = (0.3 + 0.45 * np.arange(16))[:, None, None]
        cell = 1.0 + (np.arange(333)[:, None] % 7) * 0.25 + (np.arange(33)[None, :] % 5) * 0.125
        d["taucld"] = np.asfortranarray(b * (np.array(d["cldfr"]) > 0)[None] * cell[None])
        d["inflglw"], d["iceflglw"], d["liqflglw"] = 0, 0, 0
    elif case == "mcica":
        d = make_gcm_inputs(333, 33, "cloudy", col0=40)
        d["alpha"] = np.asfortranarray(0.1 + 0.8 * np.random.default_rng(11).random((333, 33)))
    elif case == "other":
        d = make_gcm_inputs(150, 33, "cloudy", col0=900)
    else:
        raise KeyError(case)
    return d


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


_REF = {}


def _existing(hip, case, form, kind="nomcica", spectral=0, **kw):
    """Once per key: the inputs of `case` in `form` (numpy, contiguous: the call's columns and nothing else) and what the existing entry
    of that form returns on them, in that form.  spectral: 0 none, 1 total sky, 2 with the clear-sky pair - from the spectral device
    entry on the widened inputs, brought into the form with arrays.from_reference.  Shared by the tests and left unchanged."""
    form = ArrayForm(*form)
    key = (case, tuple(form), kind, spectral, tuple(sorted(kw.items())))
    if key in _REF:
        return _REF[key]
    d = _inputs(case)
    ncol, nlay = d["ncol"], d["nlay"]
    x = arrays.from_reference(d, form)
    xd = _dev(x)
    s = _stream()
    fkw = {} if form.is_reference else {"form": form}
    icld = None
    if kind == "optics":
        out = arrays.empty_like_form(OPTICS, ncol, nlay, form, hip.gpoints(), device="cuda:0", fill=float("nan"))
        hip.gas_optics_device(xd, out, stream=s, idrv=1, **fkw)
    else:
        out = arrays.empty_like_form(FLUX, ncol, nlay, form, device="cuda:0", fill=float("nan"))
        if kind == "nomcica":
            icld = hip.rrtmg_lw_device(xd, out, stream=s, **kw, **fkw)
        else:
            alpha = xd.get("alpha") if kw["icld"] in (4, 5) else None
            icld = hip.rrtmg_lw_mcica_subcol_device(xd, out, kw["seed"], kw["irng"], alpha=alpha, icld=kw["icld"], stream=s, **fkw)
    hip.check(s)
    res = _host(out)
    if spectral:
        # the spectral device entry on the widened inputs (for {8,0,0}: the existing entry of the same form itself)
        wide = arrays.to_reference(x, form)
        wd = _dev(wide)
        names = SPEC[:2] if spectral == 1 else SPEC
        so = arrays.empty_like_form(FLUX + names, ncol, nlay, REFERENCE, device="cuda:0", fill=float("nan"))
        if kind == "nomcica":
            hip.rrtmg_lw_device(wd, so, stream=s, **kw)
        else:
            alpha = wd.get("alpha") if kw["icld"] in (4, 5) else None
            hip.rrtmg_lw_mcica_subcol_device(wd, so, kw["seed"], kw["irng"], alpha=alpha, icld=kw["icld"], stream=s)
        hip.check(s)
        sh = _host(so)
        res.update(arrays.from_reference({k: sh[k] for k in names}, form))
        # (the broadband outputs of the spectral entry are those of the plain one)
        bb = arrays.from_reference({k: sh[k] for k in FLUX}, form)
        assert all(np.array_equal(bb[k], res[k], equal_nan=True) for k in FLUX)
    for v in res.values():
        v.setflags(write=False)
    _REF[key] = (x, res, icld)
    return _REF[key]


def _int(t, real_bytes):
    import torch
    return t.view(torch.int64 if real_bytes == 8 else torch.int32)


def _embed_inputs(x, form, ld, c0, names):
    """the call's input tensors as views of device fields ld wide that hold NaN everywhere else"""
    return {k: arrays.embed(_dev(np.ascontiguousarray(x[k])), k, form, ld, c0)[1] for k in names if x.get(k) is not None}


def _output_fields(names, ncol, nlay, form, ld, c0, ng=140):
    """output fields ld wide, every element the NaN pattern; returns (fields, views of the call's columns)"""
    import torch
    dt = torch.float64 if form.real_bytes == 8 else torch.float32
    fields, views = {}, {}
    for k in names:
        zero = torch.zeros(arrays.form_shape(k, ncol, nlay, form, ng), dtype=dt, device="cuda:0")
        fields[k], views[k] = arrays.embed(zero, k, form, ld, c0)
        _int(fields[k], form.real_bytes).fill_(PATTERN[form.real_bytes])
    return fields, views


def _check_outputs(fields, views, want, names, form, ncol, c0, untouched=()):
    """inside the call's columns: the reference, bit for bit; everywhere else in every field, and in all of an untouched output: the pattern"""
    for k in fields:
        f = _int(fields[k], form.real_bytes).cpu().numpy()
        outside = np.ones(f.shape, dtype=bool)
        if k not in untouched:
            arrays.field_view(outside, k, form, ncol, c0)[...] = False
        assert (f[outside] == np.array(PATTERN[form.real_bytes]).astype(f.dtype)).all(), (k, "written outside the call's columns")
    for k in names:
        got = views[k].cpu().numpy()
        assert np.isfinite(got).all(), k
        assert np.array_equal(got, want[k]), (k, tuple(form), float(np.abs(got.astype(np.float64) - want[k]).max()))


def _run_solver(hip, case, form, ld=LD, c0=C0, kind="nomcica", spectral=0, **kw):
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    x, ref, icld_ref = _existing(hip, case, form, kind, spectral, **kw)
    ncol, nlay = x["ncol"], x["nlay"]
    xin = _embed_inputs(x, form, ld or ncol, c0, _GCM_ORDER + _CLD_ORDER + ("alpha",))
    d = dict(x, **xin)
    names = FLUX + (SPEC[:2] if spectral == 1 else SPEC if spectral == 2 else ())
    fields, views = _output_fields(names, ncol, nlay, form, ld or ncol, c0)
    s = _stream()
    if kind == "nomcica":
        icld = hip.rrtmg_lw_device(d, views, stream=s, form=form, ld=ld, **kw)
    else:
        alpha = d.get("alpha") if kw["icld"] in (4, 5) else None
        icld = hip.rrtmg_lw_mcica_subcol_device(d, views, kw["seed"], kw["irng"], alpha=alpha, icld=kw["icld"], stream=s, form=form, ld=ld)
    hip.check(s)
    assert icld == icld_ref
    idrv = kw.get("idrv", x["idrv"])
    live = tuple(k for k in names if idrv == 1 or k not in FLUX[6:])
    _check_outputs(fields, views, ref, live, form, ncol, c0, untouched=tuple(k for k in names if k not in live))
    return ref


@pytest.fixture()
def batch128(hip):
    hip.set_batch(128)
    try:
        yield
    finally:
        hip.set_batch(0)


# ---- 1. rrtmg_lw_hip_run_nomcica_device_view -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("icld", [0, 1, 2])
@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_nomcica_in_a_wider_field(hip, form, icld):
    ref = _run_solver(hip, "aer_idrv", form, icld=icld)
    assert (icld == 0) == bool(np.array_equal(ref["uflx"], ref["uflxc"]))


@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_nomcica_taucld_band_by_band(hip, form):
    ref = _run_solver(hip, "inflag0", form)
    assert np.abs(ref["uflx"].astype(np.float64) - ref["uflxc"]).max() > 0.0            # the clouds are seen


@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_nomcica_several_batches_with_a_ragged_last_one(hip, batch128, form):
    assert hip.effective_batch(33) == 128
    _run_solver(hip, "aer_idrv", form)


@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_nomcica_more_than_64_layers(hip, form):
    _run_solver(hip, "tall", form, ld=201, c0=0)


@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_nomcica_columns_taken_by_cloud_top(hip, form):
    """every window of 256 columns reordered (k_colsort): the position-ordered copies of tlay, tlev and cldfr are read with the stride"""
    prev_min = hip.column_sort_min()
    prev = hip.set_column_sort(True, 0)
    try:
        _run_solver(hip, "aer_idrv", form)
    finally:
        hip.set_column_sort(prev, prev_min)


@pytest.mark.parametrize("ld", [0, 333])
@pytest.mark.parametrize("form", FORMS + [ArrayForm(4, 1, 1)], ids=fid)
def test_ld_equal_to_ncol_is_the_plain_call(hip, form, ld):
    _run_solver(hip, "aer_idrv", form, ld=ld, c0=0)


# ---- 2. the spectral outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectral", [1, 2], ids=["total", "total+clear"])
@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_spectral_outputs_in_a_wider_field(hip, form, spectral):
    ref = _run_solver(hip, "aer_idrv", form, spectral=spectral)
    assert np.abs(ref["uflxs"].astype(np.float64).sum(axis=2) - ref["uflx"]).max() < 1e-3


@pytest.mark.parametrize("spectral", [1, 2], ids=["total", "total+clear"])
def test_spectral_outputs_layer_fastest_float32_top_first(hip, spectral):
    """{4,1,1} with ld = 0: against the spectral device entry's results transposed, flipped and rounded on the host"""
    form = ArrayForm(4, 1, 1)
    ref = _run_solver(hip, "aer_idrv", form, ld=0, c0=0, spectral=spectral)
    assert ref["uflxs"].shape == (333, 34, 16) and ref["uflxs"].dtype == np.float32 and ref["uflxs"].flags.c_contiguous


def test_spectral_outputs_in_several_batches(hip, batch128):
    _run_solver(hip, "aer_idrv", R4, spectral=2)
    _run_solver(hip, "aer_idrv", R8, spectral=2)


# ---- 3. rrtmg_lw_hip_run_mcica_subcol_device_view ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("irng,icld", [(0, 2), (0, 5), (1, 2), (1, 5)])
@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_fused_mcica_in_a_wider_field(hip, form, irng, icld):
    ref = _run_solver(hip, "mcica", form, kind="mcica", seed=7, irng=irng, icld=icld)
    assert np.abs(ref["uflx"].astype(np.float64) - ref["uflxc"]).max() > 0.0


@pytest.mark.parametrize("irng", [0, 1])
def test_fused_mcica_several_batches_and_spectral(hip, batch128, irng):
    """three batches while the generator's stream - irng = 1: one over all columns of the call - runs over the whole call"""
    _run_solver(hip, "mcica", R8, kind="mcica", spectral=2, seed=7, irng=irng, icld=5)


# ---- 4. rrtmg_lw_hip_gas_optics_device_view ----------------------------------------------------------------------------------------------
def _run_optics(hip, case, form, ld, c0):
    from rrtmg_lw_amd.api import _GCM_ORDER
    x, ref, _ = _existing(hip, case, form, kind="optics")
    ncol, nlay, ng = x["ncol"], x["nlay"], hip.gpoints()
    d = dict(x, **_embed_inputs(x, form, ld, c0, _GCM_ORDER))
    fields, views = _output_fields(OPTICS, ncol, nlay, form, ld, c0, ng)
    s = _stream()
    hip.gas_optics_device(d, views, stream=s, idrv=1, form=form, ld=ld)
    hip.check(s)
    _check_outputs(fields, views, ref, OPTICS, form, ncol, c0)


@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_gas_optics_all_six_outputs(hip, form):
    _run_optics(hip, "aer_idrv", form, LD, C0)


def test_gas_optics_several_batches_and_tall(hip, batch128):
    _run_optics(hip, "aer_idrv", R8, LD, C0)
    _run_optics(hip, "tall", R4, 201, 0)


# ---- 5. rrtmg_lw_hip_adjust_tsfc_device_view ---------------------------------------------------------------------------------------------
def _adjust_reference(hip, case, form, clear):
    key = ("adjust", case, tuple(form), clear)
    if key not in _REF:
        d = _inputs(case)
        ncol, nlay = d["ncol"], d["nlay"]
        flux = _existing(hip, case, REFERENCE)[1]
        a = {k: np.array(flux[k]) for k in ADJ_IN if k in flux}
        a["plev"] = np.array(d["plev"])
        a["dtsfc"] = np.random.default_rng(21).uniform(-3.0, 3.0, ncol)
        x = arrays.from_reference(a, form)
        x.update(ncol=ncol, nlay=nlay)
        names_in = ADJ_IN if clear else ADJ_IN[:5]
        names_out = ADJ_OUT if clear else ADJ_OUT[:2]
        xd = {k: _dev(np.ascontiguousarray(x[k]) if form.layer_fastest else np.asfortranarray(x[k])) for k in names_in}
        out = arrays.empty_like_form(names_out, ncol, nlay, form, device="cuda:0", fill=float("nan"))
        s = _stream()
        hip.adjust_tsfc_device(dict(xd, ncol=ncol, nlay=nlay), out, stream=s, **({} if form.is_reference else {"form": form}))
        hip.check(s)
        res = _host(out)
        for v in res.values():
            v.setflags(write=False)
        _REF[key] = (x, res)
    return _REF[key]


def _run_adjust(hip, case, form, clear, ld, c0):
    x, ref = _adjust_reference(hip, case, form, clear)
    ncol, nlay = x["ncol"], x["nlay"]
    names_in = ADJ_IN if clear else ADJ_IN[:5]
    names_out = ADJ_OUT if clear else ADJ_OUT[:2]
    xin = _embed_inputs(x, form, ld or ncol, c0, names_in)
    fields, views = _output_fields(names_out, ncol, nlay, form, ld or ncol, c0)
    s = _stream()
    hip.adjust_tsfc_device(dict(xin, ncol=ncol, nlay=nlay), views, stream=s, form=form, ld=ld)
    hip.check(s)
    _check_outputs(fields, views, ref, names_out, form, ncol, c0)


@pytest.mark.parametrize("clear", [False, True], ids=["total", "total+clear"])
@pytest.mark.parametrize("form", FORMS, ids=fid)
def test_adjust_tsfc_in_a_wider_field(hip, form, clear):
    _run_adjust(hip, "aer_idrv", form, clear, LD, C0)           # odd offset, odd stride: one element per access


@pytest.mark.parametrize("form", [R8, R4], ids=fid)
def test_adjust_tsfc_sixteen_byte_rows(hip, form):
    """200 columns from column 8 of fields 208 wide: every row of every array starts on a 16-byte boundary - the 16-byte accesses, with
    the stride; and the same columns at an odd stride"""
    _run_adjust(hip, "tall", form, True, 208, 8)
    _run_adjust(hip, "tall", form, True, 201, 0)


def test_adjust_tsfc_layer_fastest_takes_no_stride(hip):
    _run_adjust(hip, "aer_idrv", ArrayForm(4, 1, 1), True, 0, 0)


# ---- 6. what an in-place call leaves behind ------------------------------------------------------------------------------------------------
def test_in_place_call_needs_no_more_workspace_than_the_plain_one(hip):
    x, ref, _ = _existing(hip, "aer_idrv", R8)
    hip.finalize()                                  # what earlier tests left - workspace, masks, staging - is gone
    assert hip.workspace_bytes() == 0
    hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
    try:
        xd = _dev({k: v for k, v in x.items()})
        out = arrays.empty_like_form(FLUX, 333, 33, R8, device="cuda:0")
        s = _stream()
        hip.rrtmg_lw_device(xd, out, stream=s)
        hip.check(s)
        ws_plain = hip.workspace_bytes()
        assert ws_plain > 0
        hip.finalize()
        assert hip.workspace_bytes() == 0
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)
        _run_solver(hip, "aer_idrv", R8)
        assert hip.workspace_bytes() == ws_plain
    finally:
        hip.finalize()
        hip.rrtmg_lw_ini(1004.0, kdata=hip.STANDIN_KDATA, device=0)      # (the session's fixture finalises again at the end)


def test_graph_replay_keeps_calls_of_another_ld_apart(hip):
    """A small call is captured the second time it is seen and replayed from the third on.  The same pointers with another ld are
    another call: the graph of the first must not be replayed for it."""
    import torch
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    x, ref, _ = _existing(hip, "aer_idrv", R8)
    ncol, nlay = 333, 33
    names_in, lds = _GCM_ORDER + _CLD_ORDER, (401, 403)
    size = lambda k, ld: 1 + sum((n - 1) * st for n, st in zip(arrays.form_shape(k, ncol, nlay, R8), arrays.field_strides(k, ncol, nlay, R8, ld)))
    buf = {k: torch.empty(size(k, max(lds)), dtype=torch.float64, device="cuda:0") for k in names_in + FLUX}
    view = lambda k, ld: torch.as_strided(buf[k], arrays.form_shape(k, ncol, nlay, R8), arrays.field_strides(k, ncol, nlay, R8, ld))
    s = _stream()

    def run(ld, times):
        res = []
        for k in names_in:
            buf[k].fill_(float("nan"))
            view(k, ld).copy_(_dev(np.ascontiguousarray(x[k])))
        for _ in range(times):
            for k in FLUX:
                buf[k].fill_(float("nan"))
            hip.rrtmg_lw_device(dict(x, **{k: view(k, ld) for k in names_in}), {k: view(k, ld) for k in FLUX}, stream=s, ld=ld)
            hip.check(s)
            res.append({k: view(k, ld).cpu().numpy() for k in FLUX})
        return res

    prev = hip.set_graph_max(0)
    try:
        plain = {ld: run(ld, 1)[0] for ld in lds}
    finally:
        hip.set_graph_max(prev)
    assert prev >= ncol
    for ld in lds:
        assert all(np.array_equal(plain[ld][k], ref[k]) for k in FLUX)
    c0_, r0_ = hip.graph_stats()
    first = run(lds[0], 3)
    c1_, r1_ = hip.graph_stats()
    assert c1_ == c0_ + 1 and r1_ == r0_ + 1, "the second call is captured, the third a replay"
    other = run(lds[1], 3)                                  # same pointers, another ld: its own capture, its own replay
    c2_, r2_ = hip.graph_stats()
    assert c2_ == c1_ + 1 and r2_ == r1_ + 1
    for res, ld in ((first, lds[0]), (other, lds[1])):
        for r in res:
            for k in FLUX:
                assert np.array_equal(r[k], plain[ld][k]), (ld, k)
    again = run(lds[0], 1)                                  # ... and the first one's graph is still its own
    assert hip.graph_stats()[1] == r2_ + 1
    assert all(np.array_equal(again[0][k], plain[lds[0]][k]) for k in FLUX)


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------------------
class _View(C.Structure):
    _fields_ = [("real_bytes", C.c_int), ("layer_fastest", C.c_int), ("top_first", C.c_int), ("ld", C.c_int)]


def test_bad_views_are_earg_before_anything_is_launched(hip):
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    lib = hip.lib()
    msg = lambda: lib.rrtmg_lw_hip_last_error().decode()
    x, _, _ = _existing(hip, "aer_idrv", R8)
    xin = _embed_inputs(x, R8, LD, C0, _GCM_ORDER + _CLD_ORDER)
    fields, views = _output_fields(FLUX + SPEC, 333, 33, R8, LD, C0)
    p = lambda t: C.c_void_p(t.data_ptr())

    def args(spec=SPEC, ncol=333):
        icld = C.c_int(2)
        a = [C.c_int(ncol), C.c_int(33), C.byref(icld), C.c_int(1)] + [p(xin[k]) for k in _GCM_ORDER] + [C.c_int(2), C.c_int(3), C.c_int(1)]
        a += [p(xin[k]) for k in _CLD_ORDER] + [p(views[k]) for k in FLUX]
        return a + [p(views[k]) if k in spec else C.c_void_p(0) for k in SPEC] + [C.c_void_p(0)]

    fn = lib.rrtmg_lw_hip_run_nomcica_device_view
    assert fn(None, *args()) == EARG and "view is null" in msg()
    assert fn(C.byref(_View(8, 0, 0, 332)), *args()) == EARG and "smaller than ncol" in msg()
    assert fn(C.byref(_View(8, 0, 0, -1)), *args()) == EARG and "smaller than ncol" in msg()
    assert fn(C.byref(_View(8, 1, 0, LD)), *args()) == EARG and "layer_fastest" in msg()
    assert fn(C.byref(_View(4, 1, 1, 334)), *args()) == EARG and "layer_fastest" in msg()
    assert fn(C.byref(_View(8, 0, 0, (1 << 30) + 1)), *args()) == EARG and "2^30" in msg()
    assert fn(C.byref(_View(2, 0, 0, LD)), *args()) == EARG and "real_bytes" in msg()
    for form in (_View(8, 0, 0, LD), _View(8, 0, 1, LD)):                    # in place, and through the staging
        assert fn(C.byref(form), *args(spec=("uflxs",))) == EARG and "uflxs and dflxs" in msg()
        assert fn(C.byref(form), *args(spec=("dflxs", "uflxcs"))) == EARG and "uflxs and dflxs" in msg()
        assert fn(C.byref(form), *args(spec=("uflxs", "dflxs", "dflxcs"))) == EARG and "both null or both set" in msg()
    # the other three entries check the view the same way
    m = lib.rrtmg_lw_hip_run_mcica_subcol_device_view
    irng = C.c_int(0)
    ma = args()
    ma = ma[:4] + [C.c_int(1), C.byref(irng)] + ma[4:29] + [C.c_void_p(0)] + ma[29:]        # permuteseed, irng; alpha in front of tauaer
    assert m(None, *ma) == EARG and "view is null" in msg()
    assert m(C.byref(_View(8, 0, 0, 100)), *ma) == EARG and "smaller than ncol" in msg()
    assert m(C.byref(_View(8, 1, 0, LD)), *ma) == EARG and "layer_fastest" in msg()
    g = lib.rrtmg_lw_hip_gas_optics_device_view
    oa = [C.c_int(333), C.c_int(33), C.c_int(0)] + [p(xin[k]) for k in _GCM_ORDER] + [C.c_void_p(0)] * 7
    assert g(None, *oa) == EARG and "view is null" in msg()
    assert g(C.byref(_View(8, 0, 0, 332)), *oa) == EARG and "smaller than ncol" in msg()
    assert g(C.byref(_View(8, 1, 1, LD)), *oa) == EARG and "layer_fastest" in msg()
    assert g(C.byref(_View(8, 0, 0, LD)), *oa) == EARG and "taug and fracs" in msg()
    from rrtmg_lw_amd.api import _ArrayViewC, _adjust_fn
    a = _adjust_fn("rrtmg_lw_hip_adjust_tsfc_device_view")                  # (the module declares this entry's argument types)
    aa = [333, 33] + [p(views["uflx"])] * 12 + [C.c_void_p(0)]
    assert a(None, *aa) == EARG and "view is null" in msg()
    assert a(C.byref(_ArrayViewC(4, 0, 0, 12)), *aa) == EARG and "smaller than ncol" in msg()
    assert a(C.byref(_ArrayViewC(4, 1, 0, LD)), *aa) == EARG and "layer_fastest" in msg()
    assert a(C.byref(_ArrayViewC(8, 0, 0, LD)), *aa) == EARG and "overlaps" in msg()
    hip.check(_stream())
    for k in fields:                                                        # nothing was written anywhere
        assert (_int(fields[k], 8).cpu().numpy() == PATTERN[8]).all(), k


def test_a_later_plain_call_is_unaffected(hip):
    s = _stream()
    other = _dev(_inputs("other"))
    before = arrays.empty_like_form(FLUX[:6], 150, 33, REFERENCE, device="cuda:0", fill=float("nan"))
    hip.rrtmg_lw_device(other, before, stream=s)
    hip.check(s)
    _run_solver(hip, "aer_idrv", R8)
    _run_solver(hip, "aer_idrv", R4, spectral=2)
    _run_solver(hip, "mcica", R8, kind="mcica", seed=7, irng=1, icld=5)
    after = arrays.empty_like_form(FLUX[:6], 150, 33, REFERENCE, device="cuda:0", fill=float("nan"))
    hip.rrtmg_lw_device(other, after, stream=s)
    hip.check(s)
    a, b = _host(before), _host(after)
    for k in FLUX[:6]:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
