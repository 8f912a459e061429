"""rrtmg_lw_amd.arrays: the array forms of the *_as device entries (include/rrtmg_lw_hip.h, rrtmg_lw_hip_array_form) on the CPU - the
conversions between the reference form and a form, element by element against the header's index formulas, and what the api functions
refuse before a pointer leaves Python."""
import importlib.util
import os

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import ALL_FORMS, ArrayForm
from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOL, NLAY, NG = 7, 5, 140


def _call_arrays():
    """every array class of the three entries in the reference form, every element a different number"""
    d = make_gcm_inputs(NCOL, NLAY, "aer_idrv")
    rng = np.random.default_rng(5)
    for k in ("taucld", "tauaer", "emis", "tsfc"):
        d[k] = np.asfortranarray(np.array(d[k]) + rng.random(d[k].shape))
    for k in ("alpha", "hr", "uflx", "duflx_dt", "plankbnd", "planklay", "planklev", "taug", "fracs"):
        d[k] = np.asfortranarray(rng.random(arrays.reference_shape(k, NCOL, NLAY, NG)))
    return d


def test_all_eight_forms():
    assert len(ALL_FORMS) == 8 and len(set(ALL_FORMS)) == 8 and ArrayForm(8, 0, 0).is_reference
    assert not any(f.is_reference for f in ALL_FORMS[1:])


@pytest.mark.parametrize("form", ALL_FORMS, ids=str)
def test_round_trip_is_the_identity(form):
    d = _call_arrays()
    x = arrays.from_reference(d, form)
    back = arrays.to_reference(x, form)
    again = arrays.from_reference(back, form)
    dt = np.float64 if form.real_bytes == 8 else np.float32
    for k in arrays.ALL_ARRAYS:
        if k not in d:
            continue
        assert x[k].dtype == dt and back[k].dtype == np.float64, k
        assert x[k].shape == arrays.form_shape(k, NCOL, NLAY, form, NG) and back[k].shape == d[k].shape, k
        assert x[k].flags.c_contiguous if form.layer_fastest or x[k].ndim == 1 else x[k].flags.f_contiguous, k
        assert back[k].flags.f_contiguous, k
        # to_reference o from_reference: the reference values (rounded to float32 and widened in a float32 form) ...
        assert np.array_equal(back[k], np.asarray(d[k]).astype(dt).astype(np.float64)), k
        # ... and from_reference o to_reference gives back the form's array bit for bit
        assert np.array_equal(again[k], x[k]) and again[k].dtype == x[k].dtype and again[k].strides == x[k].strides, k
    for k in ("ncol", "nlay", "icld", "idrv", "inflglw"):
        assert x[k] == d[k] and back[k] == d[k]


def _mem(a):
    """the array's values in the order they lie in memory"""
    assert a.flags.c_contiguous or a.flags.f_contiguous
    return a.ravel(order="A")


@pytest.mark.parametrize("form", ALL_FORMS, ids=str)
def test_single_elements_lie_where_the_header_says(form):
    d = _call_arrays()
    x = arrays.from_reference(d, form)
    dt = np.float64 if form.real_bytes == 8 else np.float32
    lf, top = form.layer_fastest, form.top_first
    n, L = NCOL, NLAY
    val = lambda a: dt(a)                                      # what a reference value becomes in the form
    for i, k, b, g in ((0, 0, 0, 0), (3, 1, 5, 77), (6, 4, 15, 139), (2, 3, 9, 20)):
        kk = L - 1 - k if top else k                           # layer k of the reference
        kv = L - k if top else k                               # level k of the reference (levels 0 .. nlay)
        kvt = L - (k + 1) if top else k + 1                    # ... and the top level, nlay, through the same rule
        # (ncol, nlay)
        for name in ("play", "h2ovmr", "cldfr", "alpha", "hr"):
            at = i * L + kk if lf else i + n * kk
            assert _mem(x[name])[at] == val(d[name][i, k]), (name, i, k)
        # (ncol, nlay+1)
        for name in ("plev", "tlev", "uflx", "duflx_dt"):
            at = i * (L + 1) + kv if lf else i + n * kv
            assert _mem(x[name])[at] == val(d[name][i, k]), (name, i, k)
            at = i * (L + 1) + kvt if lf else i + n * kvt
            assert _mem(x[name])[at] == val(d[name][i, k + 1]), (name, i, k + 1)
        # (ncol, 16): no vertical axis
        for name in ("emis", "plankbnd"):
            at = i * 16 + b if lf else i + n * b
            assert _mem(x[name])[at] == val(d[name][i, b]), (name, i, b)
        # taucld: (16, ncol, nlay) in the reference's order, (ncol, nlay, 16) with the layers fastest
        at = (i * L + kk) * 16 + b if lf else b + 16 * (i + n * kk)
        assert _mem(x["taucld"])[at] == val(d["taucld"][b, i, k])
        assert x["taucld"].shape == ((n, L, 16) if lf else (16, n, L))
        # tauaer, planklay: (ncol, nlay, 16), band last in both
        for name in ("tauaer", "planklay"):
            at = (i * L + kk) * 16 + b if lf else i + n * (kk + L * b)
            assert _mem(x[name])[at] == val(d[name][i, k, b]), (name, i, k, b)
        # planklev: (ncol, nlay+1, 16)
        at = (i * (L + 1) + kv) * 16 + b if lf else i + n * (kv + (L + 1) * b)
        assert _mem(x["planklev"])[at] == val(d["planklev"][i, k, b])
        # taug, fracs: (ncol, nlay, NG)
        for name in ("taug", "fracs"):
            at = (i * L + kk) * NG + g if lf else i + n * (kk + L * g)
            assert _mem(x[name])[at] == val(d[name][i, k, g]), (name, i, k, g)
        assert _mem(x["tsfc"])[i] == val(d["tsfc"][i])


def test_torch_tensors_convert_like_numpy():
    torch = pytest.importorskip("torch")
    d = _call_arrays()
    t = {k: (torch.as_tensor(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    for form in (ArrayForm(4, 1, 1), ArrayForm(8, 0, 1), ArrayForm(4, 0, 0)):
        xn, xt = arrays.from_reference(d, form), arrays.from_reference(t, form)
        bt = arrays.to_reference(xt, form)
        for k in arrays.ALL_ARRAYS:
            if k not in d:
                continue
            assert tuple(xt[k].shape) == xn[k].shape and np.array_equal(xt[k].numpy(), xn[k]), k
            # the same places in memory: strides in elements
            assert tuple(s * xt[k].element_size() for s in xt[k].stride()) == xn[k].strides, k
            assert np.array_equal(bt[k].numpy(), arrays.to_reference(xn, form)[k]), k


def test_api_refuses_tensors_that_contradict_the_form():
    """dtype -> TypeError, size / strided storage -> ValueError, before any pointer leaves Python (CPU tensors: nothing is launched)"""
    torch = pytest.importorskip("torch")
    from rrtmg_lw_amd import api
    ng = api.gpoints()
    form = ArrayForm(4, 1, 1)
    ref = make_gcm_inputs(NCOL, NLAY, "aer_idrv")
    ref["alpha"] = np.zeros((NCOL, NLAY))
    as_t = lambda x: {k: (torch.as_tensor(v) if isinstance(v, np.ndarray) else v) for k, v in x.items()}
    good = as_t(arrays.from_reference(ref, form))
    alpha = good.pop("alpha")
    out = arrays.empty_like_form(api._FLUX_OUT, NCOL, NLAY, form)
    oo = arrays.empty_like_form(api._OPTICS, NCOL, NLAY, form, ng)
    calls = {
        "nomcica": lambda d, o: api.rrtmg_lw_device(d, o, form=form),
        "mcica": lambda d, o: api.rrtmg_lw_mcica_subcol_device(d, o, 1, 0, alpha=alpha, icld=5, form=form),
        "optics": lambda d, o: api.gas_optics_device(d, oo if o is out else o, form=form),
    }
    for name, call in calls.items():
        bad = dict(good, tlay=good["tlay"].double())
        with pytest.raises(TypeError, match="'tlay'"):
            call(bad, out)
        bad = dict(good, plev=good["plev"][:, :-1].contiguous())            # nlay values per column instead of nlay + 1
        with pytest.raises(ValueError, match="'plev'"):
            call(bad, out)
        bad = dict(good, play=torch.zeros((NCOL, 2 * NLAY), dtype=torch.float32)[:, ::2])     # right size, strided
        with pytest.raises(ValueError, match="'play'"):
            call(bad, out)
    with pytest.raises(TypeError, match="'uflx'"):
        api.rrtmg_lw_device(good, dict(out, uflx=out["uflx"].double()), form=form)
    with pytest.raises(ValueError, match="'hr'"):
        api.rrtmg_lw_device(good, dict(out, hr=out["uflx"]), form=form)
    with pytest.raises(ValueError, match="'taug'"):
        api.gas_optics_device(good, dict(oo, taug=oo["planklay"]), form=form)
    with pytest.raises(TypeError, match="'alpha'"):
        api.rrtmg_lw_mcica_subcol_device(good, out, 1, 0, alpha=alpha.double(), icld=5, form=form)
    with pytest.raises(ValueError, match="bad array form"):
        api.rrtmg_lw_device(good, out, form=(2, 1, 1))
    with pytest.raises(ValueError, match="spectral"):
        api.rrtmg_lw_device(good, dict(out, uflxs=out["uflx"]), form=form)
    # a float64 reference-order form takes what the plain entry takes
    f8 = ArrayForm(8, 0, 1)
    with pytest.raises(TypeError, match="'play'"):
        api.rrtmg_lw_device(good, out, form=f8)


def test_header_declares_the_three_entries():
    spec = importlib.util.spec_from_file_location("_test_cabi", os.path.join(ROOT, "tests", "test_cabi.py"))
    cabi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cabi)
    names = cabi._declared()
    for n in ("rrtmg_lw_hip_run_nomcica_device_as", "rrtmg_lw_hip_run_mcica_subcol_device_as", "rrtmg_lw_hip_gas_optics_device_as"):
        assert n in names, n
    src = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    assert "} rrtmg_lw_hip_array_form;" in src
    from rrtmg_lw_amd import api
    assert [f[0] for f in api._ArrayFormC._fields_] == ["real_bytes", "layer_fastest", "top_first"]
