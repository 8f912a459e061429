"""Device arrays with a column stride (include/rrtmg_lw_hip.h, rrtmg_lw_hip_array_view): what can be checked without a GPU.  The
helpers of rrtmg_lw_amd.arrays that lay an array into a field `ld` columns wide and cut the call's columns out again - written from the
header's table, used by tests/test_hip_device_views.py -, the argument checks Python makes before the library is called, the size of
the view struct, the Fortran module, the exported symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd import api, arrays
from rrtmg_lw_amd.arrays import ALL_FORMS, REFERENCE, ArrayForm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
VIEW_ENTRIES = ("rrtmg_lw_hip_run_nomcica_device_view", "rrtmg_lw_hip_run_mcica_subcol_device_view",
                "rrtmg_lw_hip_gas_optics_device_view", "rrtmg_lw_hip_adjust_tsfc_device_view")
NAMES = ("play", "plev", "tsfc", "emis", "taucld", "tauaer", "planklev", "taug", "uflxs", "hr", "dtsfc")
NCOL, NLAY, NG = 7, 5, 140


def _ref_array(name, rng):
    return np.asfortranarray(rng.random(arrays.reference_shape(name, NCOL, NLAY, NG)))


@pytest.mark.parametrize("form", ALL_FORMS, ids=lambda f: "r%d_lf%d_top%d" % tuple(f))
def test_embed_and_field_view_round_trip(form):
    """an array of every kind of shape, in every form: laid into a field at a column offset, it lies where the header says (checked on
    the field's raw memory), the rest of the field holds the fill, and the view gives the array back"""
    rng = np.random.default_rng(3)
    ld, c0 = (NCOL, 0) if form.layer_fastest else (11, 3)
    dt = np.float64 if form.real_bytes == 8 else np.float32
    for name in NAMES:
        a = arrays.from_reference({name: _ref_array(name, rng)}, form)[name]
        field, view = arrays.embed(a, name, form, ld, c0, fill=-5.0)
        assert field.dtype == dt and view.shape == a.shape == arrays.form_shape(name, NCOL, NLAY, form, NG)
        assert np.array_equal(view, a) and np.shares_memory(view, field)
        assert np.array_equal(arrays.field_view(field, name, form, NCOL, c0), a)
        st = tuple(s // view.itemsize for s in view.strides)
        assert all(h == w for n, h, w in zip(view.shape, st, arrays.field_strides(name, NCOL, NLAY, form, ld, NG)) if n > 1), name
        # the header's table, on the memory itself: element (i, k) at i + ld*k, (i, k, b) at i + ld*(k + n1*b), taucld (b, i, k) at
        # b + 16*(i + ld*k), from the element of the call's first column
        if not form.layer_fastest:
            flat = field.ravel(order="F")                        # (the field is stored with its first index fastest: its memory, in order)
            assert np.shares_memory(flat, field)
            first = 16 * c0 if name == "taucld" else c0
            idx = np.indices(a.shape)
            if a.ndim == 1:
                want = first + idx[0]
            elif name == "taucld":
                want = first + idx[0] + 16 * (idx[1] + ld * idx[2])
            elif a.ndim == 2:
                want = first + idx[0] + ld * idx[1]
            else:
                want = first + idx[0] + ld * (idx[1] + a.shape[1] * idx[2])
            assert np.array_equal(flat[want], a), name
        outside = np.ones(field.shape, dtype=bool)
        arrays.field_view(outside, name, form, NCOL, c0)[...] = False
        assert (field[outside] == -5.0).all() and outside.sum() == field.size - a.size, name


def test_embed_refuses_what_does_not_fit():
    a = _ref_array("play", np.random.default_rng(0))
    with pytest.raises(ValueError, match="smaller than ncol"):
        arrays.embed(a, "play", REFERENCE, NCOL - 1)
    with pytest.raises(ValueError, match="do not lie"):
        arrays.embed(a, "play", REFERENCE, NCOL + 2, col0=3)
    lf = ArrayForm(8, 1, 0)
    with pytest.raises(ValueError, match="layer_fastest"):
        arrays.embed(arrays.from_reference({"play": a}, lf)["play"], "play", lf, NCOL + 2)
    assert arrays.check_ld(NCOL, 0, lf) == NCOL and arrays.check_ld(NCOL, None, REFERENCE) == NCOL
    with pytest.raises(ValueError, match="2\\^30"):
        arrays.check_ld(NCOL, (1 << 30) + 1, REFERENCE)


def _views(form, ld, c0, names=("play", "plev", "tsfc", "emis", "taucld", "tauaer", "uflxs")):
    import torch
    rng = np.random.default_rng(5)
    out = {}
    for name in names:
        a = arrays.from_reference({name: _ref_array(name, rng)}, form)[name]
        out[name] = arrays.embed(torch.from_numpy(np.ascontiguousarray(a)), name, form, ld, c0)[1]
    return out


def test_check_tensor_accepts_exactly_the_storage_of_the_header():
    import torch
    for form, ld, c0 in ((REFERENCE, 11, 3), (ArrayForm(4, 0, 1), 11, 0), (REFERENCE, NCOL, 0), (ArrayForm(8, 1, 0), NCOL, 0), (ArrayForm(4, 1, 1), 0, 0)):
        for name, t in _views(form, ld or NCOL, c0).items():
            arrays.check_tensor(name, t, NCOL, NLAY, form, NG, ld=ld)
            assert t.stride() == arrays.field_strides(name, NCOL, NLAY, form, ld or NCOL, NG) or 1 in t.shape
    v = _views(REFERENCE, 11, 3)
    # a view of a field of another width; a dense tensor where the call says ld = 11 (too small for it); a wrong shape; a wrong dtype
    with pytest.raises(ValueError, match="strides"):
        arrays.check_tensor("play", v["play"], NCOL, NLAY, REFERENCE, NG, ld=12)
    with pytest.raises(ValueError, match="too small for ld"):
        arrays.check_tensor("play", _views(REFERENCE, NCOL, 0)["play"], NCOL, NLAY, REFERENCE, NG, ld=11)
    with pytest.raises(ValueError, match="strides"):
        arrays.check_tensor("taucld", _views(REFERENCE, NCOL, 0)["taucld"], NCOL, NLAY, REFERENCE, NG, ld=11)
    with pytest.raises(ValueError, match="shape"):
        arrays.check_tensor("play", v["plev"], NCOL, NLAY, REFERENCE, NG, ld=11)
    with pytest.raises(ValueError, match="shape"):
        arrays.check_tensor("play", v["play"][:-1], NCOL, NLAY, REFERENCE, NG, ld=11)
    with pytest.raises(TypeError, match="float32"):
        arrays.check_tensor("play", v["play"], NCOL, NLAY, ArrayForm(4, 0, 0), NG, ld=11)
    with pytest.raises(ValueError, match="smaller than ncol"):
        arrays.check_tensor("play", v["play"], NCOL, NLAY, REFERENCE, NG, ld=NCOL - 1)
    with pytest.raises(ValueError, match="layer_fastest"):
        arrays.check_tensor("play", v["play"], NCOL, NLAY, ArrayForm(8, 1, 0), NG, ld=11)
    # without ld the check is what it was: any dense tensor of the right size
    arrays.check_tensor("play", torch.zeros(NLAY, NCOL, dtype=torch.float64), NCOL, NLAY, REFERENCE, NG)


class _Raise(Exception):
    pass


class _NoLib:
    """stands where the library would be: any entry reached means a check let the call through"""
    def __getattr__(self, name):
        if name == "rrtmg_lw_hip_gpoints":
            return lambda: NG
        raise _Raise(name)


def test_python_entries_refuse_bad_views_before_the_library_is_called(monkeypatch):
    monkeypatch.setattr(api, "lib", lambda: _NoLib())
    flux = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
    gcm = api._GCM_ORDER + api._CLD_ORDER
    names = tuple(dict.fromkeys(gcm + flux + ("alpha", "uflxs", "dflxs")))

    def call(ld, form=None, broken=None, fn="solver"):
        f = ArrayForm(*(form or REFERENCE))
        v = _views(f, NCOL if f.layer_fastest else 11, 0 if f.layer_fastest else 2, names)
        if broken:
            v[broken] = _views(f, NCOL, 0, (broken,))[broken]
        d = dict({k: v[k] for k in gcm}, ncol=NCOL, nlay=NLAY, icld=2, idrv=0, inflglw=2, iceflglw=3, liqflglw=1)
        out = {k: v[k] for k in flux + ("uflxs", "dflxs")}
        if fn == "solver":
            return api.rrtmg_lw_device(d, out, ld=ld, form=form)
        if fn == "mcica":
            return api.rrtmg_lw_mcica_subcol_device(d, out, 1, 0, alpha=v["alpha"], ld=ld, form=form)
        if fn == "optics":
            return api.gas_optics_device(d, dict(taug=None, fracs=None), ld=ld, form=form)
        return api.adjust_tsfc_device(dict(ncol=NCOL, nlay=NLAY, plev=v["plev"], dtsfc=v["tsfc"], uflx=v["uflx"], dflx=v["dflx"], duflx_dt=v["uflxc"]),
                                      dict(uflx_adj=v["dflxc"], hr_adj=v["hr"]), ld=ld, form=form)

    for fn in ("solver", "mcica", "optics", "adjust"):
        with pytest.raises(_Raise, match="_view"):              # a good call reaches the view entry, spectral outputs and all
            call(11, fn=fn)
        with pytest.raises(ValueError, match="smaller than ncol"):
            call(NCOL - 1, fn=fn)
        with pytest.raises(ValueError, match="layer_fastest"):
            call(11, form=(8, 1, 0), fn=fn)
        with pytest.raises(ValueError, match="too small for ld"):
            call(11, broken="plev", fn=fn)
    with pytest.raises(_Raise, match="_view"):                  # the spectral outputs together with a form: on the view path only
        call(11, form=(4, 0, 1))
    with pytest.raises(ValueError, match="spectral outputs are not available"):
        v = _views(REFERENCE, NCOL, 0, names)
        api.rrtmg_lw_device(dict({k: v[k] for k in gcm}, ncol=NCOL, nlay=NLAY, icld=2, idrv=0, inflglw=2, iceflglw=3, liqflglw=1),
                            {k: v[k] for k in flux + ("uflxs", "dflxs")}, form=ArrayForm(4, 0, 0))


def test_view_struct_is_sixteen_bytes():
    assert C.sizeof(api._ArrayViewC) == 16
    assert [f[0] for f in api._ArrayViewC._fields_] == ["real_bytes", "layer_fastest", "top_first", "ld"]
    src = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} rrtmg_lw_hip_array_view;", src)
    assert m and re.findall(r"int (\w+);", m.group(1)) == ["real_bytes", "layer_fastest", "top_first", "ld"]


def _declared():
    src = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rrtmg_lw_hip_\w+)\s*\(", src)))


def test_view_entries_are_declared_and_exported():
    names = _declared()
    for n in VIEW_ENTRIES:
        assert n in names, f"{n} is not declared in include/rrtmg_lw_hip.h"
    for lib in (api.lib(), C.CDLL(api.LIB_PATH_G256)):
        for n in names:
            assert hasattr(lib, n), f"{n} declared in include/rrtmg_lw_hip.h but not exported"


@pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")
def test_device_module_compiles(tmp_path):
    """module rrtmg_lw_device next to parkind and rrtmg_lw_init, and the GPU-resident host model that uses it (compile only)"""
    tmp = str(tmp_path)
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_device.f90"):
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", os.path.join(tmp, f + ".o")], check=True, cwd=tmp)
    assert os.path.exists(tmp_path / "rrtmg_lw_device.mod")
    for wp in ("8", "4"):
        subprocess.run([FLANG, "-cpp", f"-DWP={wp}", "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_device.f90"),
                        "-o", os.path.join(tmp, f"drive_device_{wp}.o")], check=True, cwd=tmp)
