"""The surface-temperature adjustment of idrv = 1 results (include/rrtmg_lw_hip.h, rrtmg_lw_hip_adjust_tsfc*; reference
src/rrtmg_lw.1col.f90:587-605): uflx_adj = uflx + duflx_dt * dtsfc, heating rates from the new net flux.  The entries are pure
arithmetic, so every comparison here is np.array_equal against the driver's lines restated in numpy float64 (_expect): the product
rounded, then the sum, the heating rate evaluated left to right.  Float32 forms: inputs widened, the same float64 arithmetic, outputs
rounded - compared as float32.

No measured figure is asserted: the kernel's time lives in profiles/adjust_tsfc.md."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import ALL_FORMS, REFERENCE, ArrayForm
from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SHIM = os.path.join(ROOT, "rrtmg_lw_amd", "fortran")
needs_flang = pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not installed")

CPDAIR = 1004.0                                            # what the session's fixture initialises the library with
HEATFAC = 9.8066 * 8.6400e4 / (CPDAIR * 1.e2)              # src/rrtmg_lw_init.f90:298
FIXTURES = ("ref_gcm_aer40_rnd", "ref_gcm_aer137")
INS = ("plev", "dtsfc", "uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")
OUTS = ("uflx_adj", "hr_adj", "uflxc_adj", "hrc_adj")
CLEAR = ("uflxc", "dflxc", "duflxc_dt", "uflxc_adj", "hrc_adj")
ENTRIES = ("rrtmg_lw_hip_adjust_tsfc", "rrtmg_lw_hip_adjust_tsfc_device", "rrtmg_lw_hip_adjust_tsfc_device_as")
EARG = 2
SENTINEL = -777.0


def _expect(d):
    """the numpy restatement on reference-form float64 arrays; clear-sky results where d holds the clear-sky inputs"""
    dt = np.asarray(d["dtsfc"], dtype=np.float64)[:, None]
    p = np.asarray(d["plev"], dtype=np.float64)
    out = {}
    for u, dn, du, ua, hr in (("uflx", "dflx", "duflx_dt", "uflx_adj", "hr_adj"), ("uflxc", "dflxc", "duflxc_dt", "uflxc_adj", "hrc_adj")):
        if d.get(u) is None:
            continue
        prod = np.asarray(d[du], dtype=np.float64) * dt              # rounded ...
        up = np.asarray(d[u], dtype=np.float64) + prod               # ... then added
        net = up - np.asarray(d[dn], dtype=np.float64)
        out[ua] = up
        out[hr] = HEATFAC * (net[:, :-1] - net[:, 1:]) / (p[:, :-1] - p[:, 1:])
    return out


def _fixture(name):
    """a reference-generated fixture's idrv = 1 results with the plev they were computed from"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=True)
    ncol, nlay = int(z["ncol"]), int(z["nlay"])
    g = make_gcm_inputs(ncol, nlay, str(z["config"]), col0=int(z["col0"]))
    d = dict(ncol=ncol, nlay=nlay, plev=np.asfortranarray(g["plev"], dtype=np.float64))
    for k in ("uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt", "hr", "hrc"):
        d[k] = np.asfortranarray(z[k], dtype=np.float64)
    return d


def _dtsfc(kind, ncol):
    if kind == "columns":
        return np.linspace(-4.0, 6.5, ncol) if ncol > 1 else np.array([2.75])
    return np.full(ncol, float(kind))


DTSFC = ("0", "1.5", "-3.25", "columns")


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_formula_with_no_change_reproduces_the_reference_heating_rates(name):
    """the yardstick itself: with dtsfc = 0 the restated lines give the reference's own hr and hrc, bit for bit"""
    d = _fixture(name)
    assert np.abs(d["duflx_dt"]).max() > 0.0 and np.abs(d["duflxc_dt"]).max() > 0.0
    got = _expect(dict(d, dtsfc=np.zeros(d["ncol"])))
    assert np.array_equal(got["uflx_adj"], d["uflx"]) and np.array_equal(got["uflxc_adj"], d["uflxc"])
    assert np.array_equal(got["hr_adj"], d["hr"])
    assert np.array_equal(got["hrc_adj"], d["hrc"])


def _header_params(name):
    src = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in include/rrtmg_lw_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_declares_the_entries_and_api_binds_them():
    from rrtmg_lw_amd import api
    want = {ENTRIES[0]: 14, ENTRIES[1]: 15, ENTRIES[2]: 16}
    for name in ENTRIES:
        params = _header_params(name)
        assert len(params) == want[name], (name, params)
        assert len(api._ADJUST_ARGTYPES[name]) == len(params), name
        assert hasattr(api.lib(), name), f"{name} is not exported"
    host, dev, as_ = (_header_params(n) for n in ENTRIES)
    assert all("double *" in p for p in host[2:]) and all(p.startswith("const") for p in host[2:10])
    assert dev[:-1] == host and dev[-1] == "void *stream"
    assert as_[0] == "const rrtmg_lw_hip_array_form *form" and as_[-1] == "void *stream"
    assert [p.split("*")[-1].strip() for p in as_[1:-1]] == [p.split("*")[-1].strip() if "*" in p else p for p in host]
    assert all(p.startswith("const void *") for p in as_[3:11]) and all(p.startswith("void *") for p in as_[11:15])
    assert callable(api.adjust_tsfc) and callable(api.adjust_tsfc_device)


def _build_fortran(tmp):
    objs = []
    for f in ("parkind.f90", "rrtmg_lw_init.f90", "rrtmg_lw_adjust.f90"):
        o = os.path.join(tmp, f + ".o")
        subprocess.run([FLANG, "-c", "-O2", "-fPIC", os.path.join(SHIM, f), "-o", o], check=True, cwd=tmp)
        objs.append(o)
    drv = os.path.join(tmp, "drive_adjust.o")
    subprocess.run([FLANG, "-c", "-O2", os.path.join(ROOT, "tests", "fortran", "drive_adjust.f90"), "-o", drv], check=True, cwd=tmp)
    return objs, drv


@needs_flang
def test_fortran_module_and_driver_compile(tmp_path):
    objs, drv = _build_fortran(str(tmp_path))
    syms = subprocess.run(["nm", objs[-1]], capture_output=True, text=True).stdout
    assert "rrtmg_lw_hip_adjust_tsfc" in syms and "rrtmg_lw_dtsfc" in syms.lower()
    assert os.path.getsize(drv) > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    """numpy array -> CUDA tensor that lies in memory exactly as the array does"""
    import torch
    t = torch.from_numpy(a).to("cuda:0")
    assert tuple(s * t.element_size() for s in t.stride()) == a.strides
    return t


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _device_call(hip, d, form=None, clear=True, stream=None):
    """the device entry (form=None) or the *_as entry on reference-form numpy inputs; returns the outputs as numpy"""
    import torch
    ncol, nlay = d["ncol"], d["nlay"]
    names_in = INS if clear else INS[:5]
    names_out = OUTS if clear else OUTS[:2]
    x = dict(ncol=ncol, nlay=nlay, **{k: _dev(np.asfortranarray(d[k], dtype=np.float64)) for k in names_in})
    out = arrays.empty_like_form(names_out, ncol, nlay, REFERENCE, device="cuda:0", fill=SENTINEL)
    s = _stream() if stream is None else stream
    hip.adjust_tsfc_device(x, out, stream=s, form=form)
    hip.check(s)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DTSFC)
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fluxes_through_the_three_entries(hip, name, kind):
    """the fixtures' real derivatives: every entry returns the numpy values; with dtsfc = 0 the reference's own uflx and hr"""
    d = _fixture(name)
    ncol, nlay = d["ncol"], d["nlay"]
    d["dtsfc"] = _dtsfc(kind, ncol)
    want = _expect(d)
    if kind == "0":
        want = dict(uflx_adj=d["uflx"], hr_adj=d["hr"], uflxc_adj=d["uflxc"], hrc_adj=d["hrc"])
    else:
        assert np.abs(want["uflx_adj"] - d["uflx"]).max() > 0.1 and np.abs(want["hr_adj"] - d["hr"]).max() > 0.0
    host = hip.adjust_tsfc(ncol, nlay, *[d[k] for k in INS])
    dev = _device_call(hip, d)
    as_ = _device_call(hip, d, form=REFERENCE)
    for k in OUTS:
        for what, got in (("host", host), ("device", dev), ("device_as", as_)):
            assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), (what, k, float(np.abs(got[k] - want[k]).max()))


def _random_case(ncol, nlay, seed=20240607):
    """reference-form float64 arrays from a seeded generator: pressures falling with height, fluxes of a few hundred W m-2"""
    rng = np.random.default_rng([seed, ncol, nlay])
    step = rng.uniform(0.2, 1.0, (ncol, nlay + 1)) * (1000.0 / (nlay + 1))
    d = dict(ncol=ncol, nlay=nlay, plev=1013.0 - np.cumsum(step, axis=1), dtsfc=rng.uniform(-5.0, 5.0, ncol))
    for k in ("uflx", "uflxc"):
        d[k] = rng.uniform(100.0, 500.0, (ncol, nlay + 1))
    for k in ("dflx", "dflxc"):
        d[k] = rng.uniform(0.0, 400.0, (ncol, nlay + 1))
    for k in ("duflx_dt", "duflxc_dt"):
        d[k] = rng.uniform(0.0, 5.0, (ncol, nlay + 1))
    return {k: (np.asfortranarray(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _flat_dev(a, pad):
    """the values of `a` as they lie in memory, inside a longer device buffer with `pad` sentinel values on either side"""
    import torch
    flat = np.ascontiguousarray(a.ravel(order="A"))
    buf = torch.full((flat.size + 2 * pad,), SENTINEL, dtype=torch.from_numpy(flat).dtype, device="cuda:0")
    buf[pad:pad + flat.size] = torch.from_numpy(flat).to("cuda:0")
    return buf, buf[pad:pad + flat.size]


def _form_call(hip, d, form, clear, pad):
    """One *_as call on the reference-form case `d` brought into `form`.  Every array lies inside a padded buffer (pad = 64 values keeps
    16-byte alignment, pad = 1 breaks it); returns the outputs in the form's shapes, the values expected there, and whether everything
    around the outputs - and the clear-sky outputs of a call without that set - kept the sentinel."""
    import torch
    ncol, nlay = d["ncol"], d["nlay"]
    dt = np.float64 if form.real_bytes == 8 else np.float32
    x = arrays.from_reference({k: d[k] for k in INS}, form)
    wide = arrays.to_reference(x, form)
    assert all(np.array_equal(wide[k], np.asarray(d[k]).astype(dt).astype(np.float64)) for k in INS)
    names_in = INS if clear else INS[:5]
    want = arrays.from_reference(_expect({k: wide[k] for k in names_in}), form)
    ins = {k: _flat_dev(x[k], pad) for k in names_in}
    outs = {k: _flat_dev(np.full(arrays.form_shape(k, ncol, nlay, form), SENTINEL, dtype=dt), pad) for k in OUTS}
    call_in = dict(ncol=ncol, nlay=nlay, **{k: v[1] for k, v in ins.items()})
    call_out = {k: v[1] for k, v in outs.items() if clear or k not in CLEAR}
    s = _stream()
    hip.adjust_tsfc_device(call_in, call_out, stream=s, form=form)
    hip.check(s)
    got, kept = {}, True
    for k, (buf, view) in outs.items():
        h = buf.cpu().numpy()
        kept = kept and bool((h[:pad] == SENTINEL).all() and (h[-pad:] == SENTINEL).all())
        body = h[pad:-pad].reshape(arrays.form_shape(k, ncol, nlay, form), order="C" if form.layer_fastest else "F")
        if k in call_out:
            got[k] = body
        else:
            kept = kept and bool((body == SENTINEL).all())
    for k, (buf, view) in ins.items():                       # inputs are read only
        kept = kept and np.array_equal(view.cpu().numpy(), np.ascontiguousarray(x[k].ravel(order="A")))
    return got, want, kept


NCOLS, NLAYS = (1, 63, 64, 65, 257), (1, 2, 40, 63, 64, 137)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ALL_FORMS, ids=lambda f: "r%d_lf%d_top%d" % tuple(f))
def test_every_form_and_ragged_shape_equals_numpy(hip, form):
    """5 column counts x 6 layer counts (nlay + 1 = 2, 64, 65; ragged waves in both mappings), with and without the clear-sky set"""
    dt = np.float64 if form.real_bytes == 8 else np.float32
    for ncol in NCOLS:
        for nlay in NLAYS:
            d = _random_case(ncol, nlay)
            for clear in (True, False):
                got, want, kept = _form_call(hip, d, form, clear, pad=64)
                assert kept, (ncol, nlay, clear, "something outside the outputs was written")
                assert sorted(got) == sorted(OUTS if clear else OUTS[:2])
                for k, v in got.items():
                    assert v.dtype == dt and want[k].dtype == dt
                    assert np.array_equal(v, want[k]), (k, ncol, nlay, clear, float(np.abs(v.astype(np.float64) - want[k]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ALL_FORMS, ids=lambda f: "r%d_lf%d_top%d" % tuple(f))
def test_arrays_off_the_16_byte_boundary(hip, form):
    """every array one value off its allocation's boundary: the kernels' one-value accesses give the same numbers"""
    for ncol, nlay in ((64, 40), (65, 63), (257, 2)):
        d = _random_case(ncol, nlay)
        got, want, kept = _form_call(hip, d, form, True, pad=1)
        assert kept
        for k, v in got.items():
            assert np.array_equal(v, want[k]), (k, ncol, nlay)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["nomcica", "fused mcica"])
def test_no_change_returns_the_solvers_own_results(hip, entry):
    """idrv = 1 through the solver, then dtsfc = 0 through the adjustment: uflx, hr, uflxc, hrc come back bit for bit"""
    import torch
    ncol, nlay = 65, 40
    d = make_gcm_inputs(ncol, nlay, "aer_idrv", col0=23)
    assert d["idrv"] == 1
    dd = {k: (_dev(np.asfortranarray(v)) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    flux = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
    o = arrays.empty_like_form(flux, ncol, nlay, REFERENCE, device="cuda:0", fill=float("nan"))
    s = _stream()
    if entry == "nomcica":
        hip.rrtmg_lw_device(dd, o, stream=s)
    else:
        hip.rrtmg_lw_mcica_subcol_device(dd, o, 11, 0, icld=2, stream=s)
    hip.check(s)
    assert float(o["duflx_dt"].abs().max()) > 0.0 and float((o["uflx"] - o["uflxc"]).abs().max()) > 0.0
    x = dict(ncol=ncol, nlay=nlay, plev=dd["plev"], dtsfc=torch.zeros(ncol, dtype=torch.float64, device="cuda:0"),
             **{k: o[k] for k in ("uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")})
    out = arrays.empty_like_form(OUTS, ncol, nlay, REFERENCE, device="cuda:0", fill=SENTINEL)
    hip.adjust_tsfc_device(x, out, stream=s)
    hip.check(s)
    for a, b in (("uflx_adj", "uflx"), ("hr_adj", "hr"), ("uflxc_adj", "uflxc"), ("hrc_adj", "hrc")):
        assert torch.equal(out[a].view(torch.int64), o[b].view(torch.int64)), (entry, a)


@pytest.mark.gpu
def test_host_entry_does_not_depend_on_batches_devices_or_pinning(hip):
    nlay = 40
    d200, d300 = _random_case(200, nlay), _random_case(300, nlay)
    ref200, ref300 = _device_call(hip, d200), _device_call(hip, d300)
    call = lambda d, **kw: hip.adjust_tsfc(d["ncol"], nlay, *[d[k] for k in INS], **kw)

    def same(got, ref, what):
        for k in OUTS:
            assert np.array_equal(got[k], ref[k]), (what, k)

    same(call(d200), ref200, "default batch")
    hip.set_batch(64)
    try:
        assert hip.effective_batch(nlay) == 64
        same(call(d200), ref200, "batches of 64")                 # 64, 64, 64, 8 columns
    finally:
        hip.set_batch(0)
    # pinned inputs and outputs: copied from and to where they lie
    pin = {k: np.asfortranarray(d200[k]).copy(order="F") for k in INS}
    shapes = dict(uflx_adj=(200, nlay + 1), hr_adj=(200, nlay), uflxc_adj=(200, nlay + 1), hrc_adj=(200, nlay))
    out = {k: np.full(shapes[k], SENTINEL, order="F") for k in OUTS}
    for a in list(pin.values()) + list(out.values()):
        hip.host_register(a)
    try:
        assert all(hip.host_is_registered(a) for a in out.values())
        got = hip.adjust_tsfc(200, nlay, *[pin[k] for k in INS], out=out)
        assert all(got[k] is out[k] for k in OUTS)
        same(got, ref200, "pinned arrays")
    finally:
        for a in list(pin.values()) + list(out.values()):
            hip.host_unregister(a)
    # without the clear-sky set nothing of it is needed or returned
    total = hip.adjust_tsfc(200, nlay, *[d200[k] for k in INS[:5]])
    assert sorted(total) == ["hr_adj", "uflx_adj"]
    assert np.array_equal(total["uflx_adj"], ref200["uflx_adj"]) and np.array_equal(total["hr_adj"], ref200["hr_adj"])
    one = call(d300)
    try:
        hip.init_devices([0, 0], kdata=hip.STANDIN_KDATA)
        assert hip.num_devices() == 2
        two = call(d300)
    finally:
        hip.rrtmg_lw_ini(CPDAIR, kdata=hip.STANDIN_KDATA, device=0)
    same(one, ref300, "one device")
    same(two, ref300, "two virtual devices")
    for k in OUTS:
        assert np.array_equal(ref200[k], _expect(d200)[k]) and np.array_equal(ref300[k], _expect(d300)[k]), k


@pytest.mark.gpu
def test_device_entry_enqueues_on_the_callers_stream_without_synchronising(hip):
    """While another stream is busy for tens of milliseconds the entry returns, its work on a side stream: had it synchronised the
    device, the other stream's work would be finished when it returns.  Results are read after check(stream)."""
    import torch
    d = _random_case(257, 63)
    want = _expect(d)
    x = dict(ncol=257, nlay=63, **{k: _dev(np.asfortranarray(d[k])) for k in INS})
    out = arrays.empty_like_form(OUTS, 257, 63, REFERENCE, device="cuda:0", fill=SENTINEL)
    busy, side = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.ones(1 << 28, dtype=torch.float32, device="cuda:0")          # 1 GiB: a pass over it is a few tenths of a millisecond
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(busy):
        for _ in range(200):
            big.mul_(1.0)
        done.record(busy)
    hip.adjust_tsfc_device(x, out, stream=side.cuda_stream)
    still_running = not done.query()
    hip.check(side.cuda_stream)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    busy.synchronize()
    assert still_running, "the entry waited for work on another stream"
    for k in OUTS:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
def test_bad_arguments_are_earg_with_a_message_and_write_nothing(hip):
    from rrtmg_lw_amd import api
    d = _random_case(65, 40)
    x = {k: _dev(np.asfortranarray(d[k])) for k in INS}
    out = arrays.empty_like_form(OUTS, 65, 40, REFERENCE, device="cuda:0", fill=SENTINEL)
    msg = lambda: hip.lib().rrtmg_lw_hip_last_error().decode()
    dev = api._adjust_fn(ENTRIES[1])
    as_ = api._adjust_fn(ENTRIES[2])
    _Form = api._ArrayFormC

    def args(nlay=40, **swap):
        p = {**{k: x[k].data_ptr() for k in INS}, **{k: out[k].data_ptr() for k in OUTS}}
        p.update(swap)
        return [65, nlay] + [C.c_void_p(p[k]) for k in INS + OUTS] + [C.c_void_p(0)]

    assert dev(*args(plev=0)) == EARG and "null input" in msg()
    assert dev(*args(hrc_adj=0)) == EARG and "4 of 5" in msg()
    assert dev(*args(duflxc_dt=0)) == EARG and "all null or all set" in msg()
    assert dev(*args(uflx_adj=x["uflx"].data_ptr())) == EARG and "uflx_adj overlaps input uflx" in msg()
    assert dev(*args(hr_adj=x["dflx"].data_ptr() + 64)) == EARG and "overlaps" in msg()
    assert dev(*args(nlay=0)) == EARG and "dimensions" in msg()
    assert as_(C.byref(_Form(2, 0, 0)), *args()) == EARG and "real_bytes" in msg()
    assert as_(None, *args()) == EARG and "form" in msg()
    assert as_(C.byref(_Form(4, 1, 1)), *args(uflxc=0)) == EARG and "all null or all set" in msg()
    # the host entry checks the same things
    h = {k: np.asfortranarray(d[k]) for k in INS}
    ho = dict(uflx_adj=h["uflx"], hr_adj=np.full((65, 40), SENTINEL, order="F"), uflxc_adj=np.full((65, 41), SENTINEL, order="F"),
              hrc_adj=np.full((65, 40), SENTINEL, order="F"))
    before = h["uflx"].copy()
    with pytest.raises(hip.RrtmgLwError, match="error %d.*overlaps" % EARG):
        hip.adjust_tsfc(65, 40, *[h[k] for k in INS], out=ho)
    assert np.array_equal(h["uflx"], before) and all((ho[k] == SENTINEL).all() for k in OUTS[1:])
    hip.check(_stream())
    assert all(bool((v == SENTINEL).all()) for v in out.values())          # nothing was written
    # ... and the library goes on working
    got = _device_call(hip, d)
    assert np.array_equal(got["hr_adj"], _expect(d)["hr_adj"])


@needs_flang
@pytest.mark.gpu
def test_fortran_host_model_gets_the_numpy_values(tmp_path, hip):
    """tests/fortran/drive_adjust.f90 on the arrays of the reference-value test: once with the optional clear-sky arguments, once without"""
    tmp = str(tmp_path)
    objs, drv = _build_fortran(tmp)
    exe = os.path.join(tmp, "drive_adjust")
    libdir = os.path.join(ROOT, "rrtmg_lw_amd")
    subprocess.run([FLANG, "-o", exe, drv, *objs, f"-L{libdir}", "-lrrtmg_lw_hip", f"-Wl,-rpath,{libdir}"], check=True, cwd=tmp)
    cases = []
    for name in FIXTURES:
        for kind in DTSFC:
            d = _fixture(name)
            d["dtsfc"] = _dtsfc(kind, d["ncol"])
            cases.append(d)
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        np.array([len(cases)], dtype=np.int32).tofile(f)
        for d in cases:
            np.array([d["ncol"], d["nlay"]], dtype=np.int32).tofile(f)
            for k in INS:
                f.write(np.asfortranarray(d[k], dtype=np.float64).tobytes(order="F"))
    env = dict(os.environ, RRTMG_LW_STATIC_TABLES=os.path.join(ROOT, "rrtmg_lw_amd", "data", "lw_static.bin"),
               RRTMG_LW_KDATA=os.path.join(ROOT, "rrtmg_lw_amd", "data", "standin.kdata.bin"))
    subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, env=env, cwd=tmp, timeout=300)
    a = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.float64)
    pos = 0
    for d in cases:
        ncol, nlay = d["ncol"], d["nlay"]
        want = _expect(d)
        for k in ("uflx_adj", "hr_adj", "uflxc_adj", "hrc_adj", "uflx_adj", "hr_adj"):      # the second call: total sky only
            shape = (ncol, nlay + 1) if k.startswith("u") else (ncol, nlay)
            n = ncol * shape[1]
            got = a[pos:pos + n].reshape(shape, order="F")
            pos += n
            assert np.array_equal(got, want[k]), (k, ncol, nlay)
    assert pos == a.size
