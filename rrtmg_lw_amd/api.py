"""Python host-side mirror of the reference's GCM interface, over the C ABI of librrtmg_lw_hip.so.

    rrtmg_lw_ini(cpdair)                         reference: src/rrtmg_lw_init.f90:47
    rrtmg_lw(ncol, nlay, icld, idrv, play, ...)  reference: src/rrtmg_lw_rad.nomcica.f90:99-108

Same names, argument order and meaning as the Fortran; arrays are numpy float64 in Fortran order (or anything
convertible).  Outputs are returned in a dict instead of being written into caller arrays.  There is no CPU
path: importing works anywhere, but every call raises unless the HIP library is built and a GPU is present.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRTMG_LW_HIP_LIB", os.path.join(_HERE, "librrtmg_lw_hip.so"))   # env override: tuning builds
STATIC_BLOB = os.path.join(_HERE, "data", "lw_static.bin")
STANDIN_KDATA = os.path.join(_HERE, "data", "standin.kdata.bin")
REAL_KDATA = os.path.join(os.path.dirname(_HERE), "data", "rrtmg_lw.kdata.bin")
NBND, NGPT = 16, 140

LIB_PATH_G256 = os.path.join(_HERE, "librrtmg_lw_hip_g256.so")      # the 256-g-point build (every band keeps its 16 original g-points)

_dp = C.POINTER(C.c_double)
_lib = None
_libs = {}
_gpoints = 140
_initialised = False


class RrtmgLwError(RuntimeError):
    pass


def lib():
    """Load the selected library - librrtmg_lw_hip.so, or librrtmg_lw_hip_g256.so after select_gpoints(256) - and fail loudly when it has
    not been built.  A process that also uses PyTorch must import torch first (one HIP runtime per process: INTEGRATION.md 2)."""
    global _lib
    if _lib is None:
        path = LIB_PATH if _gpoints == 140 else LIB_PATH_G256
        if path not in _libs:
            if not os.path.exists(path):
                raise RrtmgLwError(f"{path} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                   "(hipcc --offload-arch=gfx950); there is no CPU fallback")
            h = C.CDLL(path)
            h.rrtmg_lw_hip_last_error.restype = C.c_char_p
            h.rrtmg_lw_hip_workspace_bytes.restype = C.c_longlong
            _libs[path] = h
        _lib = _libs[path]
    return _lib


def select_gpoints(n):
    """Choose the g-point model of the calls that follow: 140 (the reference's shipped model) or 256 (every band keeps its 16 original
    g-points: the accuracy mode of modules/parrrtm.f90:40-41,77-110; its McICA arrays hold 256 sub-columns).  Each is its own library with its own
    state: call rrtmg_lw_ini after switching."""
    global _lib, _gpoints
    if n not in (140, 256):
        raise ValueError("gpoints must be 140 or 256")
    _gpoints, _lib = n, None


def gpoints():
    return int(lib().rrtmg_lw_hip_gpoints())


def _check(rc):
    if rc != 0:
        raise RrtmgLwError(f"rrtmg_lw_hip error {rc}: {lib().rrtmg_lw_hip_last_error().decode()}")


def default_kdata():
    """Real absorption coefficients if they have been converted into data/rrtmg_lw.kdata.bin
    (rrtmg_lw_amd/kdata.py); otherwise the synthetic stand-in tables - with a warning, because every flux computed
    from them is non-physical (right shapes and magnitudes only).  Pass kdata=STANDIN_KDATA explicitly (tests, bench)
    or set RRTMG_LW_ALLOW_STANDIN=1 to silence it."""
    if os.path.exists(REAL_KDATA):
        return REAL_KDATA
    if os.environ.get("RRTMG_LW_ALLOW_STANDIN", "") != "1":
        import warnings
        warnings.warn(f"{REAL_KDATA} not found: rrtmg_lw_ini falls back to the STAND-IN absorption coefficients - fluxes and "
                      "heating rates will be non-physical.  Convert the AER data with `python -m rrtmg_lw_amd.kdata "
                      "<rrtmg_lw_k_g.f90 | rrtmg_lw.nc> data/rrtmg_lw.kdata.bin`.", RuntimeWarning, stacklevel=3)
    return STANDIN_KDATA


def rrtmg_lw_ini(cpdair=1004.0, kdata=None, device=None, static=STATIC_BLOB):
    """rrtmg_lw_ini(cpdair): one-time table setup on this process's GPU (reference src/rrtmg_lw_init.f90:47).
    kdata=None: the converted real coefficients, or (with a RuntimeWarning) the stand-in tables; kdata_is_standin() tells."""
    global _initialised
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    kdata = kdata or default_kdata()
    _check(lib().rrtmg_lw_hip_init(static.encode(), kdata.encode(), C.c_double(cpdair), C.c_int(device)))
    _initialised = True


def kdata_is_standin():
    return lib().rrtmg_lw_hip_kdata_is_standin() == 1


def set_batch(n):
    _check(lib().rrtmg_lw_hip_set_batch(C.c_int(int(n))))


def effective_batch(nlay):
    """columns per internal batch in force for a call of `nlay` layers (rrtmg_lw_hip_effective_batch): the default by the call's layers or
    set_batch's size, halved until the sweeps' row offsets stay inside their buffer descriptors"""
    return int(lib().rrtmg_lw_hip_effective_batch(C.c_int(int(nlay))))


def host_register(a):
    """Pin a numpy array that will be passed to the host-pointer entries repeatedly (rrtmg_lw_hip_host_register)."""
    _check(lib().rrtmg_lw_hip_host_register(C.c_void_p(a.ctypes.data), C.c_longlong(a.nbytes)))


def host_is_registered(a):
    """whether the host-pointer entries would copy the numpy array `a` from where it lies (it is inside a range pinned by host_register)"""
    return bool(lib().rrtmg_lw_hip_host_is_registered(C.c_void_p(a.ctypes.data), C.c_longlong(a.nbytes)))


def host_unregister(a):
    _check(lib().rrtmg_lw_hip_host_unregister(C.c_void_p(a.ctypes.data)))


def host_static(a):
    """Declare the numpy array `a` static: the host-pointer entries scan its rows once instead of on every call (rrtmg_lw_hip_host_static);
    call host_changed(a) after modifying it."""
    _check(lib().rrtmg_lw_hip_host_static(C.c_void_p(a.ctypes.data), C.c_longlong(a.nbytes)))


def host_changed(a, keep=True):
    """the static array `a` has new contents (keep=False: the declaration is withdrawn as well)"""
    _check(lib().rrtmg_lw_hip_host_changed(C.c_void_p(a.ctypes.data), C.c_int(1 if keep else 0)))


def combine_stats():
    """(calls, device passes) of the combining entry for concurrent small calls since the library was loaded"""
    c, p = C.c_longlong(0), C.c_longlong(0)
    lib().rrtmg_lw_hip_combine_stats.restype = None
    lib().rrtmg_lw_hip_combine_stats(C.byref(c), C.byref(p))
    return int(c.value), int(p.value)


def set_n1_prototype(on):
    """Measurement only: cloud-free calls through the prototype of the one-column-per-wavefront mapping (k_n1)."""
    _check(lib().rrtmg_lw_hip_set_n1_prototype(C.c_int(1 if on else 0)))


def init_devices(devices, cpdair=1004.0, kdata=None, static=STATIC_BLOB):
    """rrtmg_lw_ini for several GPUs driven by this one process (rrtmg_lw_hip_init_devices): the host-pointer entries split their
    columns over `devices` (HIP ordinals; an ordinal may repeat: virtual devices on one GPU)."""
    global _initialised
    kdata = kdata or default_kdata()
    arr = (C.c_int * len(devices))(*[int(v) for v in devices])
    _check(lib().rrtmg_lw_hip_init_devices(static.encode(), kdata.encode(), C.c_double(cpdair), C.c_int(len(devices)), arr))
    _initialised = True


def last_device_state():
    """index of the library state (rrtmg_lw_hip_init_devices) this thread's last device-pointer entry ran on"""
    return int(lib().rrtmg_lw_hip_last_device_state())


def num_devices():
    return int(lib().rrtmg_lw_hip_num_devices())


def set_overlap(on):
    _check(lib().rrtmg_lw_hip_set_overlap(C.c_int(1 if on else 0)))


def set_cu_partition(layer_cus):
    """k_layer of batch i+1 on `layer_cus` CUs beside the sweeps of batch i on the others (rrtmg_lw_hip_set_cu_partition); 0 = off"""
    _check(lib().rrtmg_lw_hip_set_cu_partition(C.c_int(int(layer_cus))))


def workspace_bytes():
    """device memory the library holds right now (rrtmg_lw_hip_workspace_bytes)"""
    lib().rrtmg_lw_hip_workspace_bytes.restype = C.c_longlong
    return int(lib().rrtmg_lw_hip_workspace_bytes())


def set_one_sweep_max(ncol):
    """cloudy batches of up to `ncol` columns take one sweep launch per band group instead of three (0 = never); returns the previous value"""
    return int(lib().rrtmg_lw_hip_set_one_sweep_max(C.c_int(int(ncol))))


def set_layer_split(on):
    """k_layer's bands of a (window, layer) over several workgroups where the batch does not fill the chip (rrtmg_lw_hip_set_layer_split); returns the previous value"""
    return int(lib().rrtmg_lw_hip_set_layer_split(C.c_int(1 if on else 0)))


def set_split_max(ncol):
    """batches of up to `ncol` columns are swept one band per workgroup (rrtmg_lw_hip_set_split_max; 0 = never); returns the previous value"""
    return int(lib().rrtmg_lw_hip_set_split_max(C.c_int(int(ncol))))


def set_graph_max(ncol):
    """device-resident one-batch calls of up to `ncol` columns are replayed as one graph (rrtmg_lw_hip_set_graph_max; 0 = never); returns the previous value"""
    return int(lib().rrtmg_lw_hip_set_graph_max(C.c_int(int(ncol))))


def graph_stats():
    """(graphs captured, calls replayed from a graph) since initialisation"""
    a, b = C.c_longlong(0), C.c_longlong(0)
    lib().rrtmg_lw_hip_graph_stats(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def kiss_tables_built():
    """jump tables of the kissvec generator built so far (rrtmg_lw_hip_kiss_tables_built): does not move in steady state"""
    fn = lib().rrtmg_lw_hip_kiss_tables_built
    fn.restype = C.c_longlong
    return int(fn())


def _samples(nsamp, seedstep, **refused):
    """The sample count and seed step of a fused McICA call (include/rrtmg_lw_hip.h, "The mean over several sub-column samples"):
    -> (nsamp, seedstep) as ints, seedstep=None the sub-columns of a sample.  The averaging entries exist for float64 reference-form
    arrays only: with nsamp > 1 any of `refused` that is set raises ValueError, before the library is touched."""
    nsamp = int(nsamp)
    if nsamp > 1:
        for name, value in refused.items():
            if value is not None and value is not False:
                raise ValueError(f"nsamp = {nsamp}: the mean over several samples is not available with {name}")
    if nsamp == 1:
        return 1, 0                  # (the existing entries: they take no seedstep)
    return nsamp, (gpoints() if seedstep is None else int(seedstep))


def set_wide_window(on):
    """k_layer's second pass with the wide staging window for workgroups whose columns lie more than one reference-pressure plane apart
    (rrtmg_lw_hip_set_wide_window); returns the previous on / off"""
    return int(lib().rrtmg_lw_hip_set_wide_window(C.c_int(1 if on else 0)))


def set_column_sort(on, min_gain=-1):
    """columns of a cloudy batch (rtrn, rtrnmr, McICA) are taken by cloud top within windows of 256 where that removes >= min_gain block-levels from the
    cloud zone (rrtmg_lw_hip_set_column_sort; min_gain < 0 keeps the threshold); returns the previous on / off"""
    return int(lib().rrtmg_lw_hip_set_column_sort(C.c_int(1 if on else 0), C.c_int(int(min_gain))))


def column_sort_min():
    """the threshold of set_column_sort in force"""
    return int(lib().rrtmg_lw_hip_column_sort_min())


def set_column_sort_clear(percent):
    """what a block that the column order leaves without any cloud adds to its window's gain, in per cent of nlay block-levels
    (rrtmg_lw_hip_set_column_sort_clear); returns the previous value"""
    return int(lib().rrtmg_lw_hip_set_column_sort_clear(C.c_int(int(percent))))


def column_sort_clear():
    """the bonus of set_column_sort_clear in force"""
    return int(lib().rrtmg_lw_hip_column_sort_clear())


def set_clear_groups(on):
    """cloud-free block groups of a cloudy batch take the one clear-sky sweep launch of a cloud-free call (rrtmg_lw_hip_set_clear_groups);
    returns the previous on / off"""
    return int(lib().rrtmg_lw_hip_set_clear_groups(C.c_int(1 if on else 0)))


def cu_partition():
    return int(lib().rrtmg_lw_hip_cu_partition())


def _f(a, shape, dtype=np.float64):
    """`a` as a Fortran-ordered array of `dtype` (one that already is, is passed in place: a registered array stays registered)"""
    a = np.asfortranarray(a, dtype=dtype)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"array has shape {a.shape}, interface declares {shape}")
    return a


def _p(a):
    """the array's address (float32 arrays of the *_r4 entries too: the functions are called without argtypes, only the address passes)"""
    return a.ctypes.data_as(_dp)


def _out_ok(a, shape, name, dtype=np.float64):
    """an array the library writes into in place: of `dtype`, Fortran-contiguous, writeable, exactly the interface's shape"""
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.f_contiguous and a.flags.writeable and tuple(a.shape) == tuple(shape)):
        raise ValueError(f"output array {name!r} must be a writeable {np.dtype(dtype).name} Fortran-ordered array of shape {tuple(shape)}")
    return a


def _real(dtype, spectral=False):
    """The element type of a host call: float64 (None: the default) or float32 - the *_r4 entries of the C ABI (include/rrtmg_lw_hip.h,
    "_r4"): every array of the call is then float32, inputs are taken as Fortran-ordered float32 arrays, outputs are float32, and the
    results are the float64 call's on the widened inputs, rounded.  No spectral outputs with float32."""
    dt = np.dtype(np.float64 if dtype is None else dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype must be numpy float64 or float32, not {dt}")
    if dt == np.float32 and spectral:
        raise ValueError("the spectral outputs are not available with dtype=float32")
    return dt


_SPEC = ("uflxs", "dflxs", "uflxcs", "dflxcs")


def _spec_ptrs(out, ncol, nlay):
    """Pointers to the spectral outputs (include/rrtmg_lw_hip.h, "Spectral (per-band) fluxes"): per band the flux it adds to the
    broadband one, (ncol, nlay+1, 16) Fortran order, band 16 in the broadband call's convention.  Arrays missing from `out` are created
    there; the caller's are checked like every output (_out_ok).  uflxcs = dflxcs = None: total sky only."""
    shape = (ncol, nlay + 1, NBND)
    for k in _SPEC:
        if k not in out:
            out[k] = np.empty(shape, order="F")
    if (out["uflxcs"] is None) != (out["dflxcs"] is None):
        raise ValueError("spectral outputs: uflxcs and dflxcs must be both None or both arrays")
    return [C.cast(None, _dp) if out[k] is None and k in ("uflxcs", "dflxcs") else _p(_out_ok(out[k], shape, k)) for k in _SPEC]


def _spec_dev(out):
    """device variants: the spectral tensors' addresses (uflxcs / dflxcs may be None or absent: total sky only)"""
    return [C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else C.c_void_p(0) for k in _SPEC]


def rrtmg_lw(ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr,
             cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp,
             cliqwp, reice, reliq, tauaer, out=None, spectral=False, dtype=None):
    """Non-McICA rrtmg_lw with host arrays.  Returns dict(uflx, dflx, hr, uflxc, dflxc, hrc[, duflx_dt, duflxc_dt], icld);
    `out` may hold preallocated (e.g. host_register'ed) Fortran-ordered output arrays.  spectral=True: the dict also holds the fluxes
    per band, uflxs, dflxs, uflxcs, dflxcs of shape (ncol, nlay+1, 16) (_spec_ptrs).  dtype=np.float32: float32 arrays in and out
    (_real); without it a float32 input is widened to float64 like any other convertible array."""
    dt = _real(dtype, spectral)
    a2 = [_f(x, (ncol, nlay), dt) for x in (play,)] + [_f(plev, (ncol, nlay + 1), dt), _f(tlay, (ncol, nlay), dt),
                                                      _f(tlev, (ncol, nlay + 1), dt), _f(tsfc, (ncol,), dt)]
    gases = [_f(x, (ncol, nlay), dt) for x in (h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr)]
    em = _f(emis, (ncol, NBND), dt)
    cld = [_f(cldfr, (ncol, nlay), dt), _f(taucld, (NBND, ncol, nlay), dt), _f(cicewp, (ncol, nlay), dt), _f(cliqwp, (ncol, nlay), dt),
           _f(reice, (ncol, nlay), dt), _f(reliq, (ncol, nlay), dt), _f(tauaer, (ncol, nlay, NBND), dt)]
    if out is None:
        out = _out_arrays(ncol, nlay, idrv, dt)
    else:
        for k in ("uflx", "dflx", "uflxc", "dflxc") + (("duflx_dt", "duflxc_dt") if idrv == 1 else ()):
            _out_ok(out[k], (ncol, nlay + 1), k, dt)
        for k in ("hr", "hrc"):
            _out_ok(out[k], (ncol, nlay), k, dt)
    icld_c = C.c_int(int(icld))
    null = C.cast(None, _dp)
    args = [C.c_int(ncol), C.c_int(nlay), C.byref(icld_c), C.c_int(int(idrv))]
    args += [_p(x) for x in a2] + [_p(x) for x in gases] + [_p(em)]
    args += [C.c_int(int(inflglw)), C.c_int(int(iceflglw)), C.c_int(int(liqflglw))]
    args += [_p(x) for x in cld]
    args += [_p(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
    args += [_p(out["duflx_dt"]) if idrv == 1 else null, _p(out["duflxc_dt"]) if idrv == 1 else null]
    if spectral:
        _check(lib().rrtmg_lw_hip_run_nomcica_spectral(*args, *_spec_ptrs(out, ncol, nlay)))
    elif dt == np.float32:
        _check(lib().rrtmg_lw_hip_run_nomcica_r4(*args))
    else:
        _check(lib().rrtmg_lw_hip_run_nomcica(*args))
    out["icld"] = icld_c.value
    return out


_GCM_ORDER = ("play", "plev", "tlay", "tlev", "tsfc", "h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr",
              "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr", "emis")
_CLD_ORDER = ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq", "tauaer")
_FLUX_OUT = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")


def rrtmg_lw_from_dict(d, icld=None, idrv=None, out=None, spectral=False, dtype=None):
    """Convenience: call rrtmg_lw with the dictionaries produced by rrtmg_lw_amd.synth.make_gcm_inputs."""
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    return rrtmg_lw(d["ncol"], d["nlay"], icld, idrv, *[d[k] for k in _GCM_ORDER], d["inflglw"], d["iceflglw"],
                    d["liqflglw"], *[d[k] for k in _CLD_ORDER], out=out, spectral=spectral, dtype=dtype)


class _ArrayFormC(C.Structure):
    """rrtmg_lw_hip_array_form"""
    _fields_ = [("real_bytes", C.c_int), ("layer_fastest", C.c_int), ("top_first", C.c_int)]


def _form_arg(form, d, out, in_names, out_names):
    """The `form` argument of a *_as entry (rrtmg_lw_amd.arrays.ArrayForm), after checking every tensor the call hands over against it:
    dtype (TypeError), number of elements and dense storage (ValueError)."""
    from . import arrays
    form = arrays.ArrayForm(*form)
    if form.real_bytes not in (4, 8) or form.layer_fastest not in (0, 1) or form.top_first not in (0, 1):
        raise ValueError(f"bad array form {tuple(form)}")
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    for src, names in ((d, in_names), (out, out_names)):
        for k in names:
            if src.get(k) is not None:
                arrays.check_tensor(k, src[k], ncol, nlay, form, gpoints())
    return C.byref(_ArrayFormC(*form))


class _ArrayViewC(C.Structure):
    """rrtmg_lw_hip_array_view"""
    _fields_ = [("real_bytes", C.c_int), ("layer_fastest", C.c_int), ("top_first", C.c_int), ("ld", C.c_int)]


def _view_arg(form, ld, d, out, in_names, out_names):
    """The `view` argument of a *_view entry: the array form (None: the reference form) and ld, the column extent of the fields the
    call's tensors are views of (rrtmg_lw_amd.arrays: shapes and strides of such views; 0 = ncol).  Every tensor the call hands over is
    checked against it before the library is called - dtype (TypeError); ld < ncol, ld with layer_fastest = 1, a tensor that is not the
    call's columns of a field ld wide (ValueError)."""
    from . import arrays
    form = arrays.ArrayForm(*(form if form is not None else arrays.REFERENCE))
    if form.real_bytes not in (4, 8) or form.layer_fastest not in (0, 1) or form.top_first not in (0, 1):
        raise ValueError(f"bad array form {tuple(form)}")
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    ld = arrays.check_ld(ncol, ld, form)
    for src, names in ((d, in_names), (out, out_names)):
        for k in names:
            if src.get(k) is not None:
                arrays.check_tensor(k, src[k], ncol, nlay, form, gpoints(), ld=ld)
    return C.byref(_ArrayViewC(*form, ld))


def _spec_view(out):
    """the four spectral arguments of a solver *_view entry: null unless `out` holds them"""
    return [C.c_void_p(out[k].data_ptr()) if out.get(k) is not None else C.c_void_p(0) for k in _SPEC]


def rrtmg_lw_device(d, out, icld=None, idrv=None, stream=None, form=None, ld=None):
    """Device-resident call: `d` holds torch CUDA tensors laid out column-fastest (synth.make_gcm_inputs(backend="torch")),
    `out` a dict of preallocated output tensors (uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt).
    Enqueues on `stream` (an integer hipStream_t handle, e.g. torch.cuda.current_stream().cuda_stream) and returns
    immediately; call check(stream) to synchronise and collect physics errors.  When `out` holds uflxs (and dflxs, optionally
    uflxcs / dflxcs: (ncol, nlay+1, 16) laid out column-fastest, band last) the spectral entry fills them as well.
    form: an rrtmg_lw_amd.arrays.ArrayForm - the tensors of `d` and `out` then lie in that form (float32, (ncol, nlay) C order, top
    first: see arrays.py) and rrtmg_lw_hip_run_nomcica_device_as takes them as they are; no spectral outputs.
    ld: an integer - the call goes to rrtmg_lw_hip_run_nomcica_device_view: every tensor of `d` and `out` is a VIEW of the call's
    d["ncol"] columns inside a column-fastest field ld columns wide (a host's (pcols, pver) fields, a column range of a wider field;
    arrays.py states the shapes and strides, arrays.embed / field_view make such views; ld=0 means ncol), in `form` if one is given.
    Nothing outside the views is read or written.  The spectral outputs are available on this path in every form."""
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    icld_c = C.c_int(int(icld))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [C.c_int(d["ncol"]), C.c_int(d["nlay"]), C.byref(icld_c), C.c_int(int(idrv))]
    if ld is not None:
        view = _view_arg(form, ld, d, out, _GCM_ORDER + _CLD_ORDER, _FLUX_OUT + _SPEC)
        args = [view] + args + [ptr(d[k]) for k in _GCM_ORDER]
        args += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
        args += [ptr(d[k]) for k in _CLD_ORDER]
        args += [ptr(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
        args += [ptr(out[k]) if out.get(k) is not None else C.c_void_p(0) for k in ("duflx_dt", "duflxc_dt")]
        _check(lib().rrtmg_lw_hip_run_nomcica_device_view(*args, *_spec_view(out), C.c_void_p(stream or 0)))
        return icld_c.value
    if form is not None:
        if "uflxs" in out:
            raise ValueError("the spectral outputs are not available with an array form")
        args.insert(0, _form_arg(form, d, out, _GCM_ORDER + _CLD_ORDER, _FLUX_OUT))
    args += [ptr(d[k]) for k in _GCM_ORDER]
    args += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
    args += [ptr(d[k]) for k in _CLD_ORDER]
    args += [ptr(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
    args += [ptr(out[k]) if out.get(k) is not None else C.c_void_p(0) for k in ("duflx_dt", "duflxc_dt")]      # needed only with idrv = 1
    if "uflxs" in out:
        _check(lib().rrtmg_lw_hip_run_nomcica_spectral_device(*args, *_spec_dev(out), C.c_void_p(stream or 0)))
        return icld_c.value
    args.append(C.c_void_p(stream or 0))
    if form is not None:
        _check(lib().rrtmg_lw_hip_run_nomcica_device_as(*args))
        return icld_c.value
    _check(lib().rrtmg_lw_hip_run_nomcica_device(*args))
    return icld_c.value


def mcica_subcol_device(d, sub, icld, permuteseed, irng, alpha=None, stream=None):
    """Device-resident mcica_subcol_lw: `d` as for rrtmg_lw_device (play, cldfr, cicewp, cliqwp, reice, reliq, taucld), `sub` a dict of
    preallocated torch tensors cldfmcl, ciwpmcl, clwpmcl, taucmcl (g fastest: shape (nlay, ncol, 140) contiguous) and reicmcl, relqmcl."""
    irng_c = C.c_int(int(irng))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [C.c_int(d["ncol"]), C.c_int(d["nlay"]), C.c_int(int(icld)), C.c_int(int(permuteseed)), C.byref(irng_c)]
    args += [ptr(d[k]) for k in ("play", "cldfr", "cicewp", "cliqwp", "reice", "reliq", "taucld")]
    args += [ptr(alpha) if alpha is not None else C.c_void_p(0)]
    args += [ptr(sub[k]) for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "taucmcl")]
    args.append(C.c_void_p(stream or 0))
    _check(lib().rrtmg_lw_hip_mcica_subcol_device(*args))
    return irng_c.value


def rrtmg_lw_mcica_device(d, sub, out, icld=None, idrv=None, stream=None):
    """Device-resident McICA rrtmg_lw with explicit sub-column arrays (the reference's argument list, src/rrtmg_lw_rad.f90:99-108)."""
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    icld_c = C.c_int(int(icld))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [C.c_int(d["ncol"]), C.c_int(d["nlay"]), C.byref(icld_c), C.c_int(int(idrv))]
    args += [ptr(d[k]) for k in _GCM_ORDER]
    args += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
    args += [ptr(sub[k]) for k in ("cldfmcl", "taucmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl")] + [ptr(d["tauaer"])]
    args += [ptr(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
    args += [ptr(out[k]) if out.get(k) is not None else C.c_void_p(0) for k in ("duflx_dt", "duflxc_dt")]      # needed only with idrv = 1
    if "uflxs" in out:          # spectral outputs (see rrtmg_lw_device)
        _check(lib().rrtmg_lw_hip_run_mcica_spectral_device(*args, *_spec_dev(out), C.c_void_p(stream or 0)))
        return icld_c.value
    args.append(C.c_void_p(stream or 0))
    _check(lib().rrtmg_lw_hip_run_mcica_device(*args))
    return icld_c.value


def check(stream=None):
    _check(lib().rrtmg_lw_hip_check(C.c_void_p(stream or 0)))


def run_columns(cols, istart=1, iend=16, icld=None, idrv=None):
    """Prepared-column entry for a list of column dicts (rrtmg_lw_amd.io_rrtm.read_input_rrtm) that share nlayers
    and cloud flags.  Returns dict of arrays (ncol, 0:nlayers)."""
    n = len(cols)
    nl = int(cols[0]["nlayers"])
    icld = int(cols[0]["icld"]) if icld is None else icld
    idrv = int(cols[0]["idrv"]) if idrv is None else idrv
    st = lambda key, shape: _f(np.stack([np.asarray(c[key], dtype=np.float64).reshape(shape[1:], order="F") for c in cols]), shape)
    a = dict(pavel=st("pavel", (n, nl)), tavel=st("tavel", (n, nl)), pz=st("pz", (n, nl + 1)), tz=st("tz", (n, nl + 1)),
             tbound=_f(np.array([float(c["tbound"]) for c in cols]), (n,)), semiss=st("semiss", (n, NBND)),
             coldry=st("coldry", (n, nl)), wkl=st("wkl", (n, 7, nl)), wbrodl=st("wbrodl", (n, nl)), wx=st("wx", (n, 4, nl)),
             pwvcm=_f(np.array([float(c["pwvcm"]) for c in cols]), (n,)), cldfrac=st("cldfrac", (n, nl)),
             tauc=st("tauc", (n, NBND, nl)), ciwp=st("ciwp", (n, nl)), clwp=st("clwp", (n, nl)), rei=st("rei", (n, nl)),
             rel=st("rel", (n, nl)), taua=st("tauaer", (n, nl, NBND)))
    names = ("totuflux", "totdflux", "fnet", "htr", "totuclfl", "totdclfl", "fnetc", "htrc", "dtotuflux_dt", "dtotuclfl_dt")
    out = {k: np.zeros((n, nl + 1), order="F") for k in names}
    c0 = cols[0]
    args = [C.c_int(n), C.c_int(nl), C.c_int(istart), C.c_int(iend), C.c_int(icld), C.c_int(idrv)]
    args += [_p(a[k]) for k in ("pavel", "tavel", "pz", "tz", "tbound", "semiss", "coldry", "wkl", "wbrodl", "wx", "pwvcm")]
    args += [C.c_int(int(c0["inflag"])), C.c_int(int(c0["iceflag"])), C.c_int(int(c0["liqflag"]))]
    args += [_p(a[k]) for k in ("cldfrac", "tauc", "ciwp", "clwp", "rei", "rel", "taua")]
    args += [_p(out[k]) for k in names]
    _check(lib().rrtmg_lw_hip_run_columns(*args))
    return out


# ---------------------------------------------------------------------------------------------------
# Gas optics and Planck sources (include/rrtmg_lw_hip.h, "Gas optics and Planck sources")
# ---------------------------------------------------------------------------------------------------
_OPTICS = ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt")


def _optics_shapes(ncol, nlay):
    ng = gpoints()
    return dict(taug=(ncol, nlay, ng), fracs=(ncol, nlay, ng), planklay=(ncol, nlay, NBND), planklev=(ncol, nlay + 1, NBND),
                plankbnd=(ncol, NBND), dplankbnd_dt=(ncol, NBND))


def _optics_ptrs(out, ncol, nlay, idrv):
    """pointers to the gas-optics outputs of `out` (created there where missing; dplankbnd_dt only with idrv = 1); a Planck output the
    caller sets to None is not formed"""
    shapes = _optics_shapes(ncol, nlay)
    for k in _OPTICS:
        if k not in out and (k != "dplankbnd_dt" or idrv == 1):
            out[k] = np.empty(shapes[k], order="F")
    for k in ("taug", "fracs"):
        if out[k] is None:
            raise ValueError(f"gas optics: {k} is required")
    return [_p(_out_ok(out[k], shapes[k], k)) if out.get(k) is not None else C.cast(None, _dp) for k in _OPTICS]


def gas_optics(d, idrv=0, out=None):
    """Gas optical depth and Planck fraction per g-point, Planck integrals per band (rrtmg_lw_hip_gas_optics) for the GCM inputs of
    rrtmg_lw_from_dict (cloud and aerosol entries of `d` are not used).  Returns a dict of Fortran-ordered arrays: taug, fracs
    (ncol, nlay, ngpt), planklay (ncol, nlay, 16), planklev (ncol, nlay+1, 16), plankbnd (ncol, 16) and, with idrv = 1, dplankbnd_dt
    (ncol, 16).  `out` may hold preallocated arrays; a Planck output set to None there is not formed."""
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    a = _gcm_arrays(ncol, nlay, *[d[k] for k in ("play", "plev", "tlay", "tlev", "tsfc")],
                    [d[k] for k in _GCM_ORDER[5:15]], d["emis"])
    out = {} if out is None else out
    ptrs = _optics_ptrs(out, ncol, nlay, idrv)
    _check(lib().rrtmg_lw_hip_gas_optics(C.c_int(ncol), C.c_int(nlay), C.c_int(int(idrv)), *[_p(x) for x in a], *ptrs))
    return out


def gas_optics_device(d, out, stream=None, idrv=None, form=None, ld=None):
    """Device-resident gas optics (rrtmg_lw_hip_gas_optics_device): `d` as for rrtmg_lw_device (torch tensors, column fastest), `out` a
    dict of preallocated float64 tensors laid out column fastest, g-point / band last - taug, fracs of shape (ngpt, nlay, ncol), planklay
    (16, nlay, ncol), planklev (16, nlay+1, ncol), plankbnd, dplankbnd_dt (16, ncol); the Planck ones optional.  Enqueues on `stream`
    and returns; call check(stream) to synchronise.  idrv: d["idrv"] unless given.  form: as for rrtmg_lw_device - with layer_fastest
    taug and fracs are (ncol, nlay, ngpt) C-contiguous, planklay (ncol, nlay, 16), planklev (ncol, nlay+1, 16), plankbnd (ncol, 16).
    ld: as for rrtmg_lw_device (rrtmg_lw_hip_gas_optics_device_view) - the tensors are views of the call's columns in fields ld wide,
    with the logical shapes of arrays.py: taug, fracs (ncol, nlay, ngpt), planklay (ncol, nlay, 16), planklev (ncol, nlay+1, 16)."""
    idrv = d["idrv"] if idrv is None else idrv
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    args = [C.c_int(d["ncol"]), C.c_int(d["nlay"]), C.c_int(int(idrv))] + [ptr(d[k]) for k in _GCM_ORDER]
    args += [ptr(out.get(k)) for k in _OPTICS]
    if ld is not None:
        view = _view_arg(form, ld, d, out, _GCM_ORDER, _OPTICS)
        _check(lib().rrtmg_lw_hip_gas_optics_device_view(view, *args, C.c_void_p(stream or 0)))
        return
    if form is not None:
        _check(lib().rrtmg_lw_hip_gas_optics_device_as(_form_arg(form, d, out, _GCM_ORDER, _OPTICS), *args, C.c_void_p(stream or 0)))
        return
    _check(lib().rrtmg_lw_hip_gas_optics_device(*args, C.c_void_p(stream or 0)))


def gas_optics_columns(cols, idrv=0, out=None):
    """Gas optics for prepared columns (rrtmg_lw_hip_gas_optics_columns): `cols` as for run_columns (at most one batch).  Returns the
    dict of gas_optics."""
    n = len(cols)
    nl = int(cols[0]["nlayers"])
    st = lambda key, shape: _f(np.stack([np.asarray(c[key], dtype=np.float64).reshape(shape[1:], order="F") for c in cols]), shape)
    a = [st("pavel", (n, nl)), st("tavel", (n, nl)), st("pz", (n, nl + 1)), st("tz", (n, nl + 1)),
         _f(np.array([float(c["tbound"]) for c in cols]), (n,)), st("semiss", (n, NBND)), st("coldry", (n, nl)), st("wkl", (n, 7, nl)),
         st("wbrodl", (n, nl)), st("wx", (n, 4, nl)), _f(np.array([float(c["pwvcm"]) for c in cols]), (n,))]
    out = {} if out is None else out
    ptrs = _optics_ptrs(out, n, nl, idrv)
    _check(lib().rrtmg_lw_hip_gas_optics_columns(C.c_int(n), C.c_int(nl), C.c_int(int(idrv)), *[_p(x) for x in a], *ptrs))
    return out


# ---------------------------------------------------------------------------------------------------
# Surface-temperature adjustment of idrv = 1 results (include/rrtmg_lw_hip.h, "Surface-temperature adjustment")
# ---------------------------------------------------------------------------------------------------
_ADJUST_IN = ("plev", "dtsfc", "uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")
_ADJUST_OUT = ("uflx_adj", "hr_adj", "uflxc_adj", "hrc_adj")
_ADJUST_CLEAR = ("uflxc", "dflxc", "duflxc_dt", "uflxc_adj", "hrc_adj")
# the argument lists of the three C entries as this module passes them (tests/test_adjust_tsfc.py holds them against the header)
_ADJUST_ARGTYPES = {
    "rrtmg_lw_hip_adjust_tsfc": [C.c_int, C.c_int] + [_dp] * 12,
    "rrtmg_lw_hip_adjust_tsfc_r4": [C.c_int, C.c_int] + [C.POINTER(C.c_float)] * 12,
    "rrtmg_lw_hip_adjust_tsfc_device": [C.c_int, C.c_int] + [C.c_void_p] * 13,
    "rrtmg_lw_hip_adjust_tsfc_device_as": [C.POINTER(_ArrayFormC), C.c_int, C.c_int] + [C.c_void_p] * 13,
    "rrtmg_lw_hip_adjust_tsfc_device_view": [C.POINTER(_ArrayViewC), C.c_int, C.c_int] + [C.c_void_p] * 13,
}


def _adjust_fn(name):
    fn = getattr(lib(), name)
    fn.argtypes, fn.restype = _ADJUST_ARGTYPES[name], C.c_int
    return fn


def adjust_tsfc(ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, uflxc=None, dflxc=None, duflxc_dt=None, out=None, dtype=None):
    """The fluxes and heating rates of an idrv = 1 radiation call adjusted to a changed surface temperature (rrtmg_lw_hip_adjust_tsfc;
    reference src/rrtmg_lw.1col.f90:582-610), host arrays: uflx_adj = uflx + duflx_dt * dtsfc, hr_adj from the new net flux.  dtsfc
    (ncol,) is the current surface temperature minus the tsfc of that call; uflx, dflx, duflx_dt are its stored, unadjusted results.
    The clear-sky arrays uflxc, dflxc, duflxc_dt are all given or all None.  Returns dict(uflx_adj (ncol, nlay+1), hr_adj (ncol, nlay)
    [, uflxc_adj, hrc_adj]); `out` may hold preallocated (e.g. host_register'ed) Fortran-ordered arrays of those names.
    dtype=np.float32: float32 arrays in and out (rrtmg_lw_hip_adjust_tsfc_r4; _real)."""
    ncol, nlay = int(ncol), int(nlay)
    dt = _real(dtype)
    r4 = dt == np.float32
    ptr = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))) if r4 else _p
    clear = (uflxc, dflxc, duflxc_dt)
    if any(x is None for x in clear) and not all(x is None for x in clear):
        raise ValueError("adjust_tsfc: uflxc, dflxc and duflxc_dt must be all None or all arrays")
    has_c = clear[0] is not None
    lev, lay = (ncol, nlay + 1), (ncol, nlay)
    null = C.cast(None, C.POINTER(C.c_float) if r4 else _dp)
    ins = [_f(plev, lev, dt), _f(dtsfc, (ncol,), dt)] + [_f(x, lev, dt) for x in (uflx, dflx, duflx_dt)] + ([_f(x, lev, dt) for x in clear] if has_c else [])
    out = {} if out is None else out
    shapes = dict(uflx_adj=lev, hr_adj=lay, uflxc_adj=lev, hrc_adj=lay)
    names = _ADJUST_OUT if has_c else _ADJUST_OUT[:2]
    for k in names:
        if k not in out:
            out[k] = np.empty(shapes[k], dtype=dt, order="F")
        _out_ok(out[k], shapes[k], k, dt)
    o = [ptr(out[k]) if k in names else null for k in _ADJUST_OUT]
    fn = _adjust_fn("rrtmg_lw_hip_adjust_tsfc_r4" if r4 else "rrtmg_lw_hip_adjust_tsfc")
    _check(fn(ncol, nlay, *[ptr(x) for x in ins], *([null] * 3 if not has_c else []), *o))
    return out


def adjust_tsfc_device(arrays, out, stream=None, form=None, ld=None):
    """Device-resident adjustment (rrtmg_lw_hip_adjust_tsfc_device): `arrays` holds ncol, nlay and the torch CUDA tensors plev, dtsfc,
    uflx, dflx, duflx_dt and - all or none - uflxc, dflxc, duflxc_dt, laid out column fastest as for rrtmg_lw_device; `out` the
    preallocated tensors uflx_adj, hr_adj and, with the clear-sky inputs, uflxc_adj, hrc_adj.  One kernel launch on `stream`, no
    synchronisation: check(stream) before the results are read.  form: an rrtmg_lw_amd.arrays.ArrayForm - every tensor then lies in
    that form (dtsfc in its precision) and is read and written where it lies (rrtmg_lw_hip_adjust_tsfc_device_as).  ld: as for
    rrtmg_lw_device (rrtmg_lw_hip_adjust_tsfc_device_view) - the tensors are views of the call's columns in fields ld wide."""
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    args = [int(arrays["ncol"]), int(arrays["nlay"])] + [ptr(arrays.get(k)) for k in _ADJUST_IN] + [ptr(out.get(k)) for k in _ADJUST_OUT]
    if ld is not None:
        view = _view_arg(form, ld, arrays, out, _ADJUST_IN, _ADJUST_OUT)
        _check(_adjust_fn("rrtmg_lw_hip_adjust_tsfc_device_view")(view, *args, C.c_void_p(stream or 0)))
        return
    if form is not None:
        _check(_adjust_fn("rrtmg_lw_hip_adjust_tsfc_device_as")(_form_arg(form, arrays, out, _ADJUST_IN, _ADJUST_OUT), *args, C.c_void_p(stream or 0)))
        return
    _check(_adjust_fn("rrtmg_lw_hip_adjust_tsfc_device")(*args, C.c_void_p(stream or 0)))


# ---------------------------------------------------------------------------------------------------
# McICA flavour: reference src/rrtmg_lw_rad.f90:99-108, src/mcica_subcol_gen_lw.f90:68,183
# ---------------------------------------------------------------------------------------------------
def _out_arrays(ncol, nlay, idrv, dtype=np.float64):
    out = {k: np.empty((ncol, nlay + 1), dtype=dtype, order="F") for k in ("uflx", "dflx", "uflxc", "dflxc")}
    out["hr"] = np.empty((ncol, nlay), dtype=dtype, order="F")
    out["hrc"] = np.empty((ncol, nlay), dtype=dtype, order="F")
    if idrv == 1:
        out["duflx_dt"] = np.empty((ncol, nlay + 1), dtype=dtype, order="F")
        out["duflxc_dt"] = np.empty((ncol, nlay + 1), dtype=dtype, order="F")
    return out


def _out_ptrs(out, idrv):
    null = C.cast(None, _dp)
    return [_p(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")] + \
           [_p(out["duflx_dt"]) if idrv == 1 else null, _p(out["duflxc_dt"]) if idrv == 1 else null]


def _gcm_arrays(ncol, nlay, play, plev, tlay, tlev, tsfc, gases, emis, dt=np.float64):
    return [_f(play, (ncol, nlay), dt), _f(plev, (ncol, nlay + 1), dt), _f(tlay, (ncol, nlay), dt), _f(tlev, (ncol, nlay + 1), dt),
            _f(tsfc, (ncol,), dt)] + [_f(x, (ncol, nlay), dt) for x in gases] + [_f(emis, (ncol, NBND), dt)]


def rrtmg_lw_mcica(ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr,
                   cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, cldfmcl, taucmcl, ciwpmcl,
                   clwpmcl, reicmcl, relqmcl, tauaer, spectral=False, out=None, dtype=None):
    """McICA rrtmg_lw (src/rrtmg_lw_rad.f90:99-108) with host arrays; sub-column arrays are (140, ncol, nlay).
    spectral=True: the fluxes per band as well (see rrtmg_lw); `out`: a dict of preallocated spectral outputs to fill.
    dtype=np.float32: float32 arrays in and out (rrtmg_lw_hip_run_mcica_r4; _real)."""
    dt = _real(dtype, spectral)
    a = _gcm_arrays(ncol, nlay, play, plev, tlay, tlev, tsfc,
                    (h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr), emis, dt)
    ng = gpoints()
    cld = [_f(cldfmcl, (ng, ncol, nlay), dt), _f(taucmcl, (ng, ncol, nlay), dt), _f(ciwpmcl, (ng, ncol, nlay), dt),
           _f(clwpmcl, (ng, ncol, nlay), dt), _f(reicmcl, (ncol, nlay), dt), _f(relqmcl, (ncol, nlay), dt), _f(tauaer, (ncol, nlay, NBND), dt)]
    out = dict(out or {}, **_out_arrays(ncol, nlay, idrv, dt))
    icld_c = C.c_int(int(icld))
    args = [C.c_int(ncol), C.c_int(nlay), C.byref(icld_c), C.c_int(int(idrv))] + [_p(x) for x in a]
    args += [C.c_int(int(inflglw)), C.c_int(int(iceflglw)), C.c_int(int(liqflglw))] + [_p(x) for x in cld] + _out_ptrs(out, idrv)
    if spectral:
        _check(lib().rrtmg_lw_hip_run_mcica_spectral(*args, *_spec_ptrs(out, ncol, nlay)))
    elif dt == np.float32:
        _check(lib().rrtmg_lw_hip_run_mcica_r4(*args))
    else:
        _check(lib().rrtmg_lw_hip_run_mcica(*args))
    out["icld"] = icld_c.value
    return out


_MC_ORDER = ("cldfmcl", "taucmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "tauaer")


def rrtmg_lw_mcica_from_dict(d, icld=None, idrv=None, spectral=False, out=None, dtype=None):
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    return rrtmg_lw_mcica(d["ncol"], d["nlay"], icld, idrv, *[d[k] for k in _GCM_ORDER], d["inflglw"], d["iceflglw"],
                          d["liqflglw"], *[d[k] for k in _MC_ORDER], spectral=spectral, out=out, dtype=dtype)


def get_alpha(ncol, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac):
    """get_alpha (src/mcica_subcol_gen_lw.f90:68): decorrelation-length overlap parameter, (ncol, nlay)."""
    alpha = np.zeros((ncol, nlay), order="F")
    _check(lib().rrtmg_lw_hip_get_alpha(C.c_int(ncol), C.c_int(nlay), C.c_int(int(icld)), C.c_int(int(idcor)),
                                        C.c_double(float(decorr_con)), _p(_f(dz, (ncol, nlay))), _p(_f(lat, (ncol,))),
                                        C.c_int(int(juldat)), _p(_f(cldfrac, (ncol, nlay))), _p(alpha)))
    return alpha


def mcica_subcol_lw(ncol, nlay, icld, permuteseed, irng, play, cldfrac, ciwp, clwp, rei, rel, tauc, alpha=None, out=None):
    """mcica_subcol_lw (src/mcica_subcol_gen_lw.f90:183-185; `iplon` dropped: every column is generated).
    Returns dict(cldfmcl, ciwpmcl, clwpmcl, taucmcl (ngpt,ncol,nlay), reicmcl, relqmcl (ncol,nlay), irng); `out`: such a dict of
    preallocated Fortran-ordered arrays to fill (a host model's sub-column arrays persist)."""
    ng = gpoints()
    z3 = lambda: np.zeros((ng, ncol, nlay), order="F")
    z2 = lambda: np.zeros((ncol, nlay), order="F")
    o = out if out is not None else dict(cldfmcl=z3(), ciwpmcl=z3(), clwpmcl=z3(), reicmcl=z2(), relqmcl=z2(), taucmcl=z3())
    # the C entry writes through these pointers: every output must BE a float64 Fortran-ordered array of the declared shape (_f would
    # silently hand a converted copy to nobody)
    for k, shape in (("cldfmcl", (ng, ncol, nlay)), ("ciwpmcl", (ng, ncol, nlay)), ("clwpmcl", (ng, ncol, nlay)), ("taucmcl", (ng, ncol, nlay)),
                     ("reicmcl", (ncol, nlay)), ("relqmcl", (ncol, nlay))):
        _out_ok(o[k], shape, k)
    irng_c = C.c_int(int(irng))
    ins = [_f(play, (ncol, nlay)), _f(cldfrac, (ncol, nlay)), _f(ciwp, (ncol, nlay)), _f(clwp, (ncol, nlay)),
           _f(rei, (ncol, nlay)), _f(rel, (ncol, nlay)), _f(tauc, (NBND, ncol, nlay))]
    al = _p(_f(alpha, (ncol, nlay))) if alpha is not None else C.cast(None, _dp)
    _check(lib().rrtmg_lw_hip_mcica_subcol(C.c_int(ncol), C.c_int(nlay), C.c_int(int(icld)), C.c_int(int(permuteseed)),
                                           C.byref(irng_c), *[_p(x) for x in ins], al,
                                           *[_p(o[k]) for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl", "taucmcl")]))
    o["irng"] = irng_c.value
    return o


def rrtmg_lw_mcica_subcol(ncol, nlay, icld, idrv, permuteseed, irng, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr,
                          ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw,
                          cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, spectral=False, out=None, dtype=None,
                          nsamp=1, seedstep=None, var=False):
    """mcica_subcol_lw followed by the McICA rrtmg_lw in one call; the sub-columns stay on the device as bit masks.
    spectral=True: the fluxes per band as well (see rrtmg_lw); `out`: a dict of preallocated spectral outputs to fill.
    dtype=np.float32: float32 arrays in and out, alpha too (rrtmg_lw_hip_run_mcica_subcol_r4; _real).
    nsamp > 1: the mean of the total-sky outputs over nsamp samples drawn with permuteseed + s * seedstep (seedstep=None: gpoints()),
    summed in float64 in sample order and divided once; clear-sky outputs are sample 0's (rrtmg_lw_hip_run_mcica_samples).
    var=True (nsamp > 1, float64): the result also holds uflx_var, dflx_var, hr_var, the unbiased sample variances of uflx, dflx, hr
    over the samples (rrtmg_lw_hip_run_mcica_samples_var; the standard error of the mean is sqrt(var / nsamp))."""
    nsamp, seedstep = _samples(nsamp, seedstep, **{"spectral=True": spectral, "a float32 dtype": dtype is not None and np.dtype(dtype) == np.float32})
    if var and nsamp == 1:
        raise ValueError("var=True with nsamp = 1: the sample variance needs at least two samples")
    dt = _real(dtype, spectral)
    a = _gcm_arrays(ncol, nlay, play, plev, tlay, tlev, tsfc,
                    (h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr), emis, dt)
    keep = [_f(cldfr, (ncol, nlay), dt), _f(taucld, (NBND, ncol, nlay), dt), _f(cicewp, (ncol, nlay), dt), _f(cliqwp, (ncol, nlay), dt),
            _f(reice, (ncol, nlay), dt), _f(reliq, (ncol, nlay), dt), _f(alpha, (ncol, nlay), dt) if alpha is not None else None,
            _f(tauaer, (ncol, nlay, NBND), dt)]
    cld = [_p(x) if x is not None else C.cast(None, _dp) for x in keep]
    out = dict(out or {}, **_out_arrays(ncol, nlay, idrv, dt))
    icld_c, irng_c = C.c_int(int(icld)), C.c_int(int(irng))
    args = [C.c_int(ncol), C.c_int(nlay), C.byref(icld_c), C.c_int(int(idrv)), C.c_int(int(permuteseed)), C.byref(irng_c)]
    if nsamp != 1:
        args[5:5] = [C.c_int(nsamp), C.c_int(seedstep)]
    args += [_p(x) for x in a] + [C.c_int(int(inflglw)), C.c_int(int(iceflglw)), C.c_int(int(liqflglw))] + cld + _out_ptrs(out, idrv)
    if var:
        out.update(uflx_var=np.empty((ncol, nlay + 1), order="F"), dflx_var=np.empty((ncol, nlay + 1), order="F"), hr_var=np.empty((ncol, nlay), order="F"))
        _check(lib().rrtmg_lw_hip_run_mcica_samples_var(*args, *[_p(out[k]) for k in _VAR_OUT]))
    elif nsamp != 1:
        _check(lib().rrtmg_lw_hip_run_mcica_samples(*args))
    elif spectral:
        _check(lib().rrtmg_lw_hip_run_mcica_subcol_spectral(*args, *_spec_ptrs(out, ncol, nlay)))
    elif dt == np.float32:
        _check(lib().rrtmg_lw_hip_run_mcica_subcol_r4(*args))
    else:
        _check(lib().rrtmg_lw_hip_run_mcica_subcol(*args))
    out["icld"] = icld_c.value
    out["irng"] = irng_c.value
    return out


def rrtmg_lw_mcica_subcol_from_dict(d, permuteseed, irng, alpha=None, icld=None, idrv=None, spectral=False, out=None, dtype=None,
                                    nsamp=1, seedstep=None, var=False):
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    return rrtmg_lw_mcica_subcol(d["ncol"], d["nlay"], icld, idrv, permuteseed, irng, *[d[k] for k in _GCM_ORDER], d["inflglw"],
                                 d["iceflglw"], d["liqflglw"], d["cldfr"], d["taucld"], d["cicewp"], d["cliqwp"], d["reice"],
                                 d["reliq"], alpha, d["tauaer"], spectral=spectral, out=out, dtype=dtype, nsamp=nsamp, seedstep=seedstep, var=var)


def rrtmg_lw_mcica_subcol_device(d, out, permuteseed, irng, alpha=None, icld=None, idrv=None, stream=None, form=None, ld=None,
                                 nsamp=1, seedstep=None):
    """Device-resident fused generator + solver (torch CUDA tensors, column-fastest); see rrtmg_lw_device (`form` and `ld` as there:
    `alpha` lies in that form, and is such a view, as well; ld goes to rrtmg_lw_hip_run_mcica_subcol_device_view).
    nsamp, seedstep: as in rrtmg_lw_mcica_subcol (rrtmg_lw_hip_run_mcica_samples_device: float64 reference-form tensors only)."""
    nsamp, seedstep = _samples(nsamp, seedstep, **{"form=": form, "ld=": ld, "spectral outputs": "uflxs" in out,
                                                   "float32 tensors": str(getattr(out.get("uflx"), "dtype", "")).endswith("float32")})
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    icld_c, irng_c = C.c_int(int(icld)), C.c_int(int(irng))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [C.c_int(d["ncol"]), C.c_int(d["nlay"]), C.byref(icld_c), C.c_int(int(idrv)), C.c_int(int(permuteseed)), C.byref(irng_c)]
    if ld is not None:
        view = _view_arg(form, ld, dict(d, alpha=alpha), out, _GCM_ORDER + _CLD_ORDER + ("alpha",), _FLUX_OUT + _SPEC)
        args = [view] + args + [ptr(d[k]) for k in _GCM_ORDER]
        args += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
        args += [ptr(d[k]) for k in ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq")]
        args += [ptr(alpha) if alpha is not None else C.c_void_p(0), ptr(d["tauaer"])]
        args += [ptr(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
        args += [ptr(out[k]) if out.get(k) is not None else C.c_void_p(0) for k in ("duflx_dt", "duflxc_dt")]
        _check(lib().rrtmg_lw_hip_run_mcica_subcol_device_view(*args, *_spec_view(out), C.c_void_p(stream or 0)))
        return icld_c.value
    if form is not None:
        if "uflxs" in out:
            raise ValueError("the spectral outputs are not available with an array form")
        args.insert(0, _form_arg(form, dict(d, alpha=alpha), out, _GCM_ORDER + _CLD_ORDER + ("alpha",), _FLUX_OUT))
    args += [ptr(d[k]) for k in _GCM_ORDER]
    args += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
    args += [ptr(d[k]) for k in ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq")]
    args += [ptr(alpha) if alpha is not None else C.c_void_p(0), ptr(d["tauaer"])]
    args += [ptr(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
    args += [ptr(out[k]) if out.get(k) is not None else C.c_void_p(0) for k in ("duflx_dt", "duflxc_dt")]      # needed only with idrv = 1
    if "uflxs" in out:          # spectral outputs (see rrtmg_lw_device)
        _check(lib().rrtmg_lw_hip_run_mcica_subcol_spectral_device(*args, *_spec_dev(out), C.c_void_p(stream or 0)))
        return icld_c.value
    args.append(C.c_void_p(stream or 0))
    if nsamp != 1:
        args[5:5] = [C.c_int(nsamp), C.c_int(seedstep)]
        _check(lib().rrtmg_lw_hip_run_mcica_samples_device(*args))
        return icld_c.value
    if form is not None:
        _check(lib().rrtmg_lw_hip_run_mcica_subcol_device_as(*args))
        return icld_c.value
    _check(lib().rrtmg_lw_hip_run_mcica_subcol_device(*args))
    return icld_c.value


_VAR_OUT = ("uflx_var", "dflx_var", "hr_var")


def _checked_view(form, ld, ncol, nlay, tensors):
    """The `view` argument of a *_view entry, as _view_arg makes it, for a dict of named tensors (None: not given) - without a look at
    the library: the forms of these arrays do not depend on the number of g-points."""
    from . import arrays
    form = arrays.ArrayForm(*(form if form is not None else arrays.REFERENCE))
    if form.real_bytes not in (4, 8) or form.layer_fastest not in (0, 1) or form.top_first not in (0, 1):
        raise ValueError(f"bad array form {tuple(form)}")
    ld = arrays.check_ld(ncol, ld, form)
    for k, t in tensors.items():
        if t is not None:
            arrays.check_tensor(k, t, ncol, nlay, form, ld=ld)
    return C.byref(_ArrayViewC(*form, ld))


def rrtmg_lw_mcica_samples_device(d, out, permuteseed, nsamp, seedstep=None, alpha=None, icld=None, idrv=None, stream=None, form=None, ld=None):
    """Device-resident mean over nsamp sub-column samples (kissvec generator, seeds permuteseed + s * seedstep; seedstep=None:
    gpoints()) of the fused generator + solver, in the caller's own array form and width (rrtmg_lw_hip_run_mcica_samples_device_view):
    `d`, `out`, `alpha`, `form`, `ld` as in rrtmg_lw_mcica_subcol_device with ld= (ld=None: ncol - contiguous tensors of the form).
    `out` may also hold uflx_var, dflx_var, hr_var (each on its own; shapes of uflx, dflx, hr, in the form): the unbiased sample
    variances, formed where the mean is formed; the standard error of the mean is sqrt(var / nsamp).  Without them: the mean alone.
    ValueError before the library is touched: spectral outputs in `out`, a variance with nsamp = 1, tensors that are not the form's."""
    nsamp = int(nsamp)
    for k in _SPEC:
        if out.get(k) is not None:
            raise ValueError(f"'{k}': the averaging entry has no spectral outputs")
    for k in _VAR_OUT:
        if out.get(k) is not None and nsamp == 1:
            raise ValueError(f"{k} with nsamp = 1: the sample variance needs at least two samples")
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    tensors = {k: d.get(k) for k in _GCM_ORDER + _CLD_ORDER}
    tensors["alpha"] = alpha
    tensors.update({k: out.get(k) for k in _FLUX_OUT + _VAR_OUT})
    view = _checked_view(form, ld or 0, ncol, nlay, tensors)
    icld = d["icld"] if icld is None else icld
    idrv = d["idrv"] if idrv is None else idrv
    seedstep = gpoints() if seedstep is None else int(seedstep)
    icld_c, irng_c = C.c_int(int(icld)), C.c_int(0)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    args = [view, C.c_int(ncol), C.c_int(nlay), C.byref(icld_c), C.c_int(int(idrv)), C.c_int(int(permuteseed)), C.c_int(nsamp), C.c_int(seedstep),
            C.byref(irng_c)]
    args += [ptr(d[k]) for k in _GCM_ORDER]
    args += [C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
    args += [ptr(d[k]) for k in ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq")]
    args += [ptr(alpha), ptr(d["tauaer"])]
    args += [ptr(out.get(k)) for k in _FLUX_OUT + _VAR_OUT]
    _check(lib().rrtmg_lw_hip_run_mcica_samples_device_view(*args, C.c_void_p(stream or 0)))
    return icld_c.value


def get_alpha_device(d, alpha, icld, idcor, decorr_con, juldat, stream=None, form=None, ld=None):
    """Device-resident get_alpha (rrtmg_lw_hip_get_alpha_device_view): `d` holds torch CUDA tensors dz, cldfr (or cldfrac) (ncol, nlay)
    and lat (ncol,) - and ncol, nlay - in `form` (None: the reference form), views of fields `ld` columns wide if ld is given; `alpha`
    the output tensor of the same kind, which the fused McICA entries take as it is.  Enqueues on `stream`, does not synchronise; icld
    other than 4 or 5 leaves alpha alone."""
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    cldfr = d["cldfr"] if d.get("cldfr") is not None else d.get("cldfrac")
    view = _checked_view(form, ld or 0, ncol, nlay, {"dz": d.get("dz"), "lat": d.get("lat"), "cldfr": cldfr, "alpha": alpha})
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    _check(lib().rrtmg_lw_hip_get_alpha_device_view(view, C.c_int(ncol), C.c_int(nlay), C.c_int(int(icld)), C.c_int(int(idcor)),
                                                    C.c_double(float(decorr_con)), ptr(d.get("dz")), ptr(d.get("lat")), C.c_int(int(juldat)),
                                                    ptr(cldfr), ptr(alpha), C.c_void_p(stream or 0)))
    return alpha


_COVER_OUT = ("cldtot", "cldcum", "cldlay", "submask")


def mask_words():
    """32-bit words of a sub-column mask: (gpoints() + 31) // 32"""
    return (gpoints() + 31) // 32


def mcica_cloud_cover(ncol, nlay, icld, permuteseed, irng, play, cldfrac, alpha=None, nsamp=1, seedstep=None,
                      outputs=("cldtot", "cldcum", "cldlay")):
    """Cloud cover as the McICA sub-columns realise it (rrtmg_lw_hip_mcica_cloud_cover; include/rrtmg_lw_hip.h states the definitions):
    the generator stage of the fused entries with the same (icld, permuteseed, irng, play, cldfrac, alpha), counted.  numpy arrays
    (ncol, nlay) as for mcica_subcol_lw; nsamp samples with the seeds permuteseed + s * seedstep (seedstep=None: gpoints()).
    `outputs`: which of cldtot (ncol,), cldcum, cldlay (ncol, nlay) - float64 - and submask (ncol, nlay, mask_words()), uint32, nsamp = 1
    only, to form.  Returns a dict of them (Fortran-ordered) and irng as the library left it."""
    outputs = tuple(outputs)
    for k in outputs:
        if k not in _COVER_OUT:
            raise ValueError(f"unknown output {k!r}: one of {_COVER_OUT}")
    shapes = {"cldtot": (ncol,), "cldcum": (ncol, nlay), "cldlay": (ncol, nlay), "submask": (ncol, nlay, mask_words())}
    o = {k: np.zeros(shapes[k], dtype=np.uint32 if k == "submask" else np.float64, order="F") for k in outputs}
    irng_c = C.c_int(int(irng))
    null = C.cast(None, _dp)
    opt = lambda a: _p(_f(a, (ncol, nlay))) if a is not None else null
    seedstep = gpoints() if seedstep is None else int(seedstep)
    _check(lib().rrtmg_lw_hip_mcica_cloud_cover(C.c_int(ncol), C.c_int(nlay), C.c_int(int(icld)), C.c_int(int(permuteseed)),
                                                C.c_int(int(nsamp)), C.c_int(seedstep), C.byref(irng_c), opt(play), opt(cldfrac), opt(alpha),
                                                *[_p(o[k]) if k in o else null for k in _COVER_OUT]))
    o["irng"] = irng_c.value
    return o


def mcica_cloud_cover_device(d, out, icld, permuteseed, irng=0, alpha=None, nsamp=1, seedstep=None, stream=None, form=None, ld=None):
    """Device-resident mcica_cloud_cover: `d` holds torch CUDA tensors play and cldfr (ncol, nlay) - and ncol, nlay -, `alpha` the one
    of the exponential overlaps, `out` the preallocated output tensors: those of cldtot (ncol,), cldcum, cldlay (ncol, nlay) and submask
    that it holds are formed, the others are not.  form / ld as in get_alpha_device (rrtmg_lw_hip_mcica_cloud_cover_device_view); with
    neither the plain rrtmg_lw_hip_mcica_cloud_cover_device.  submask is an int32 (or uint32) tensor of logical shape
    (ncol, nlay, mask_words()): stored column-fastest - strides (1, ld, ld * nlay) -, or C-contiguous with a layer_fastest form.
    Enqueues on `stream`, does not synchronise (check(stream) collects a physics error).  Returns irng as the library left it."""
    import torch
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    for k in out:
        if k not in _COVER_OUT:
            raise ValueError(f"unknown output {k!r}: one of {_COVER_OUT}")
    cldfr = d["cldfr"] if d.get("cldfr") is not None else d.get("cldfrac")
    tensors = {"play": d.get("play"), "cldfr": cldfr, "alpha": alpha}
    tensors.update({k: out.get(k) for k in ("cldtot", "cldcum", "cldlay")})
    view = _checked_view(form, ld or 0, ncol, nlay, tensors)
    sub = out.get("submask")
    if sub is not None:
        from . import arrays
        f = arrays.ArrayForm(*(form if form is not None else arrays.REFERENCE))
        w = arrays.check_ld(ncol, ld, f)
        mw = mask_words()
        if sub.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise TypeError(f"'submask' is {sub.dtype}: 32-bit words (torch.int32 or torch.uint32)")
        need = (nlay * mw, mw, 1) if f.layer_fastest else (1, w, w * nlay)
        if tuple(sub.shape) != (ncol, nlay, mw) or any(n > 1 and a != b for n, a, b in zip(sub.shape, sub.stride(), need)):
            raise ValueError(f"'submask' has shape {tuple(sub.shape)} and strides {tuple(sub.stride())}: needs {(ncol, nlay, mw)} with strides {need}")
    seedstep = gpoints() if seedstep is None else int(seedstep)
    irng_c = C.c_int(int(irng))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    args = [C.c_int(ncol), C.c_int(nlay), C.c_int(int(icld)), C.c_int(int(permuteseed)), C.c_int(int(nsamp)), C.c_int(seedstep), C.byref(irng_c),
            ptr(d.get("play")), ptr(cldfr), ptr(alpha)] + [ptr(out.get(k)) for k in _COVER_OUT] + [C.c_void_p(stream or 0)]
    if form is None and ld is None:
        _check(lib().rrtmg_lw_hip_mcica_cloud_cover_device(*args))
    else:
        _check(lib().rrtmg_lw_hip_mcica_cloud_cover_device_view(view, *args))
    return irng_c.value


_CLOUD_OPTICS_IN = ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq", "plev", "h2ovmr")
_CLOUD_OPTICS_OUT = ("taucloud", "ncbands", "secdiff")


def _cloud_optics_needed(given):
    """the inputs a cloud-optics call reads: the six cloud arrays for taucloud or ncbands, plev and h2ovmr for secdiff"""
    if not given:
        raise ValueError(f"cloud optics: no output given - at least one of {_CLOUD_OPTICS_OUT}")
    return (_CLOUD_OPTICS_IN[:6] if ("taucloud" in given or "ncbands" in given) else ()) + (_CLOUD_OPTICS_IN[6:] if "secdiff" in given else ())


def cloud_optics(d, imca=0, out=None):
    """Cloud optical depth per spectral band before the diffusivity secant, cldprop's band count and the secants
    (rrtmg_lw_hip_cloud_optics; include/rrtmg_lw_hip.h states the definitions): imca = 0 cldprop, 1 cldprmc on a cloudy sub-column.
    `d` as for rrtmg_lw_from_dict: ncol, nlay, the three cloud flags, numpy float64 arrays cldfr, cicewp, cliqwp, reice, reliq
    (ncol, nlay), taucld (16, ncol, nlay) - for taucloud or ncbands - and plev (ncol, nlay+1), h2ovmr (ncol, nlay) - for secdiff.
    Returns a dict of Fortran-ordered arrays taucloud (ncol, nlay, 16), ncbands (ncol,) int32, secdiff (ncol, 16).  `out` may hold
    preallocated arrays; an output set to None there is not formed (and its inputs are not needed).  An array of another dtype or
    shape is refused (TypeError / ValueError), not converted."""
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    shapes = {"taucloud": (ncol, nlay, NBND), "ncbands": (ncol,), "secdiff": (ncol, NBND)}
    out = {} if out is None else out
    for k in out:
        if k not in _CLOUD_OPTICS_OUT:
            raise ValueError(f"unknown output {k!r}: one of {_CLOUD_OPTICS_OUT}")
    for k in _CLOUD_OPTICS_OUT:
        if k not in out:
            out[k] = np.zeros(shapes[k], dtype=np.int32 if k == "ncbands" else np.float64, order="F")
    given = [k for k in _CLOUD_OPTICS_OUT if out[k] is not None]
    needed = _cloud_optics_needed(given)
    in_shapes = {k: (ncol, nlay) for k in _CLOUD_OPTICS_IN}
    in_shapes.update(taucld=(NBND, ncol, nlay), plev=(ncol, nlay + 1))
    null = C.cast(None, _dp)
    ins = []
    for k in _CLOUD_OPTICS_IN:
        if k not in needed:
            ins.append(null)
            continue
        a = d.get(k)
        if not isinstance(a, np.ndarray) or a.dtype != np.float64:
            raise TypeError(f"cloud optics: {k!r} must be a numpy float64 array, not {getattr(a, 'dtype', type(a).__name__)}")
        a = _f(a, in_shapes[k])
        ins.append(a)
    outs = [_p(_out_ok(out[k], shapes[k], k, np.int32 if k == "ncbands" else np.float64)) if out[k] is not None else null for k in _CLOUD_OPTICS_OUT]
    _check(lib().rrtmg_lw_hip_cloud_optics(C.c_int(ncol), C.c_int(nlay), C.c_int(int(imca)), C.c_int(int(d["inflglw"])),
                                           C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"])),
                                           *[a if a is null else _p(a) for a in ins], *outs))
    return out


def cloud_optics_device(d, out, imca=0, stream=None, form=None, ld=None):
    """Device-resident cloud_optics: `d` holds torch CUDA tensors as for rrtmg_lw_device - of them cldfr, taucld, cicewp, cliqwp, reice,
    reliq are read for taucloud or ncbands, plev and h2ovmr for secdiff -, ncol, nlay and the three cloud flags; `out` the preallocated
    output tensors: those of taucloud (like tauaer), ncbands ((ncol,) torch.int32, whatever the form) and secdiff (like emis) that it
    holds are formed, the others are not.  form / ld as in get_alpha_device (rrtmg_lw_hip_cloud_optics_device_view; every form runs on
    the tensors in place); with neither the plain rrtmg_lw_hip_cloud_optics_device.  A tensor that is not exactly the form's - dtype,
    shape, strides - is refused.  Enqueues on `stream`, does not synchronise (check(stream) collects a particle-size stop)."""
    import torch
    ncol, nlay = int(d["ncol"]), int(d["nlay"])
    for k in out:
        if k not in _CLOUD_OPTICS_OUT:
            raise ValueError(f"unknown output {k!r}: one of {_CLOUD_OPTICS_OUT}")
    given = [k for k in _CLOUD_OPTICS_OUT if out.get(k) is not None]
    needed = _cloud_optics_needed(given)
    tensors = {k: d.get(k) for k in needed}
    for k in needed:
        if tensors[k] is None:
            raise ValueError(f"cloud optics: input {k!r} is missing")
    tensors.update({k: out.get(k) for k in ("taucloud", "secdiff")})
    view = _checked_view(form, ld or 0, ncol, nlay, tensors)
    nb = out.get("ncbands")
    if nb is not None:
        if nb.dtype != torch.int32:
            raise TypeError(f"'ncbands' is {nb.dtype}: it is torch.int32 whatever the array form")
        if tuple(nb.shape) != (ncol,) or (ncol > 1 and nb.stride(0) != 1):
            raise ValueError(f"'ncbands' has shape {tuple(nb.shape)} and strides {tuple(nb.stride())}: needs {(ncol,)}, contiguous")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    args = [C.c_int(ncol), C.c_int(nlay), C.c_int(int(imca)), C.c_int(int(d["inflglw"])), C.c_int(int(d["iceflglw"])), C.c_int(int(d["liqflglw"]))]
    args += [ptr(tensors.get(k)) for k in _CLOUD_OPTICS_IN] + [ptr(out.get(k)) for k in _CLOUD_OPTICS_OUT] + [C.c_void_p(stream or 0)]
    if form is None and ld is None:
        _check(lib().rrtmg_lw_hip_cloud_optics_device(*args))
    else:
        _check(lib().rrtmg_lw_hip_cloud_optics_device_view(view, *args))


_SOLVE_IN = ("plev", "emis", "tau", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt", "cldfr", "odcld", "submask")
_SOLVE_OUT = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")


def _solve_shapes(ncol, nlay):
    ng, mw = gpoints(), mask_words()
    ins = dict(plev=(ncol, nlay + 1), emis=(ncol, NBND), tau=(ncol, nlay, ng), fracs=(ncol, nlay, ng), planklay=(ncol, nlay, NBND),
               planklev=(ncol, nlay + 1, NBND), plankbnd=(ncol, NBND), dplankbnd_dt=(ncol, NBND), cldfr=(ncol, nlay), odcld=(ncol, nlay, NBND),
               submask=(ncol, nlay, mw))
    lev, lay = (ncol, nlay + 1), (ncol, nlay)
    outs = dict(uflx=lev, dflx=lev, hr=lay, uflxc=lev, dflxc=lev, hrc=lay, duflx_dt=lev, duflxc_dt=lev)
    return ins, outs


def _solve_needed(cloud, idrv):
    """the inputs a solve call reads"""
    return _SOLVE_IN[:7] + (("dplankbnd_dt",) if idrv == 1 else ()) + (("cldfr",) if cloud == 1 else ()) + (("odcld",) if cloud in (1, 2) else ()) + \
        (("submask",) if cloud == 2 else ())


def solve(d, cloud=0, idrv=0, out=None):
    """Fluxes and heating rates from the caller's optical depths and sources (rrtmg_lw_hip_solve; include/rrtmg_lw_hip.h states the
    recurrences): cloud = 0 no cloud, 1 rtrn on cldfr and odcld, 2 rtrnmc on submask and odcld.  `d`: ncol, nlay and Fortran-ordered
    numpy float64 arrays plev (ncol, nlay+1), emis, plankbnd (ncol, 16), tau, fracs (ncol, nlay, gpoints()), planklay (ncol, nlay, 16),
    planklev (ncol, nlay+1, 16), with idrv = 1 dplankbnd_dt (ncol, 16), with cloud = 1 cldfr (ncol, nlay), with cloud != 0 odcld
    (ncol, nlay, 16), with cloud = 2 submask (ncol, nlay, mask_words()) uint32 - the layouts gas_optics, cloud_optics and
    mcica_cloud_cover return.  Returns a dict of Fortran-ordered arrays uflx, dflx, uflxc, dflxc (ncol, nlay+1), hr, hrc (ncol, nlay) and,
    with idrv = 1, duflx_dt, duflxc_dt.  `out` may hold preallocated arrays; the clear-sky triple set to None there is not formed.
    An array of another dtype or shape is refused (TypeError / ValueError), not converted."""
    ncol, nlay, cloud, idrv = int(d["ncol"]), int(d["nlay"]), int(cloud), int(idrv)
    in_shapes, out_shapes = _solve_shapes(ncol, nlay)
    out = {} if out is None else out
    for k in out:
        if k not in _SOLVE_OUT:
            raise ValueError(f"unknown output {k!r}: one of {_SOLVE_OUT}")
    for k in _SOLVE_OUT:
        if k not in out and (idrv == 1 or not k.startswith("du")):
            out[k] = np.zeros(out_shapes[k], order="F")
    null = C.cast(None, _dp)
    ins = []
    for k in _SOLVE_IN:
        if k not in _solve_needed(cloud, idrv):
            ins.append(null)
            continue
        a, want = d.get(k), np.uint32 if k == "submask" else np.float64
        if not isinstance(a, np.ndarray) or a.dtype != want:
            raise TypeError(f"solve: {k!r} must be a numpy {np.dtype(want).name} array, not {getattr(a, 'dtype', type(a).__name__)}")
        ins.append(_f(a, in_shapes[k], dtype=want))
    outs = [_p(_out_ok(out[k], out_shapes[k], k)) if out.get(k) is not None else null for k in _SOLVE_OUT]
    _check(lib().rrtmg_lw_hip_solve(C.c_int(ncol), C.c_int(nlay), C.c_int(cloud), C.c_int(idrv), *[a if a is null else _p(a) for a in ins], *outs))
    return out


def solve_device(d, out, cloud=0, idrv=None, stream=None):
    """Device-resident solve: `d` holds ncol, nlay and torch CUDA float64 tensors in the reference form (column-fastest; submask
    torch.int32 or torch.uint32) under the names of solve, `out` the preallocated output tensors: uflx, dflx, hr, the clear-sky triple
    all or none, duflx_dt and duflxc_dt with idrv = 1 (idrv = None: 1 when `out` holds duflx_dt).  A tensor that is not exactly the
    reference form - dtype, shape, strides - is refused.  Enqueues on `stream`, does not synchronise."""
    import torch
    ncol, nlay, cloud = int(d["ncol"]), int(d["nlay"]), int(cloud)
    for k in out:
        if k not in _SOLVE_OUT:
            raise ValueError(f"unknown output {k!r}: one of {_SOLVE_OUT}")
    idrv = (1 if out.get("duflx_dt") is not None else 0) if idrv is None else int(idrv)
    in_shapes, out_shapes = _solve_shapes(ncol, nlay)
    needed = _solve_needed(cloud, idrv)

    def ok(k, t, shape):
        if k == "submask":
            if t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise TypeError(f"'submask' is {t.dtype}: 32-bit words (torch.int32 or torch.uint32)")
        elif t.dtype != torch.float64:
            raise TypeError(f"solve: {k!r} is {t.dtype}: torch.float64")
        need, s = [], 1
        for n in shape:
            need.append(s)
            s *= n
        if not t.is_cuda or tuple(t.shape) != tuple(shape) or any(n > 1 and a != b for n, a, b in zip(shape, t.stride(), need)):
            raise ValueError(f"solve: {k!r} has shape {tuple(t.shape)} and strides {tuple(t.stride())}: needs a CUDA tensor of shape {tuple(shape)} with strides {tuple(need)}")
        return t

    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    args = [C.c_int(ncol), C.c_int(nlay), C.c_int(cloud), C.c_int(idrv)]
    for k in _SOLVE_IN:
        if k in needed and d.get(k) is None:
            raise ValueError(f"solve: input {k!r} is missing")
        args.append(ptr(ok(k, d[k], in_shapes[k]) if k in needed else None))
    args += [ptr(ok(k, out[k], out_shapes[k]) if out.get(k) is not None else None) for k in _SOLVE_OUT] + [C.c_void_p(stream or 0)]
    _check(lib().rrtmg_lw_hip_solve_device(*args))


def run_columns_mcica(cols, subs, istart=1, iend=16, icld=None, idrv=None):
    """Prepared-column McICA entry: cols[k] (rrtmg_lw_amd.io_rrtm.read_input_rrtm dicts) with sub-columns subs[k] =
    dict(cldfmc, taucmc, ciwpmc, clwpmc (140, nlayers), reicmc, relqmc (nlayers)); one (column, sample) pair per entry.
    Returns dict of arrays (n, 0:nlayers)."""
    n = len(cols)
    nl = int(cols[0]["nlayers"])
    icld = int(cols[0]["icld"]) if icld is None else icld
    idrv = int(cols[0]["idrv"]) if idrv is None else idrv
    st = lambda src, key, shape: _f(np.stack([np.asarray(c[key], dtype=np.float64).reshape(shape[1:], order="F") for c in src]), shape)
    a = dict(pavel=st(cols, "pavel", (n, nl)), tavel=st(cols, "tavel", (n, nl)), pz=st(cols, "pz", (n, nl + 1)), tz=st(cols, "tz", (n, nl + 1)),
             tbound=_f(np.array([float(c["tbound"]) for c in cols]), (n,)), semiss=st(cols, "semiss", (n, NBND)),
             coldry=st(cols, "coldry", (n, nl)), wkl=st(cols, "wkl", (n, 7, nl)), wbrodl=st(cols, "wbrodl", (n, nl)), wx=st(cols, "wx", (n, 4, nl)),
             pwvcm=_f(np.array([float(c["pwvcm"]) for c in cols]), (n,)), reicmc=st(subs, "reicmc", (n, nl)), relqmc=st(subs, "relqmc", (n, nl)),
             taua=st(cols, "tauaer", (n, nl, NBND)))
    for k in ("cldfmc", "taucmc", "ciwpmc", "clwpmc"):          # (140, n, nlayers)
        a[k] = _f(np.stack([np.asarray(s_[k], dtype=np.float64) for s_ in subs], axis=1), (gpoints(), n, nl))
    names = ("totuflux", "totdflux", "fnet", "htr", "totuclfl", "totdclfl", "fnetc", "htrc", "dtotuflux_dt", "dtotuclfl_dt")
    out = {k: np.zeros((n, nl + 1), order="F") for k in names}
    c0 = cols[0]
    args = [C.c_int(n), C.c_int(nl), C.c_int(istart), C.c_int(iend), C.c_int(icld), C.c_int(idrv)]
    args += [_p(a[k]) for k in ("pavel", "tavel", "pz", "tz", "tbound", "semiss", "coldry", "wkl", "wbrodl", "wx", "pwvcm")]
    args += [C.c_int(int(c0["inflag"])), C.c_int(int(c0["iceflag"])), C.c_int(int(c0["liqflag"]))]
    args += [_p(a[k]) for k in ("cldfmc", "taucmc", "ciwpmc", "clwpmc", "reicmc", "relqmc", "taua")]
    args += [_p(out[k]) for k in names]
    _check(lib().rrtmg_lw_hip_run_columns_mcica(*args))
    return out


def column_mcica_samples(col, samples, irng=1, alpha=None):
    """The column driver's McICA loop for one prepared column (src/rrtmg_lw.1col.f90:471-660): sub-columns of sample `ims`
    from mcica_subcol_lw with permuteseed = ims * 140, then cldprmc -> rtrnmc; returns the per-sample results (n, 0:nlayers)
    and the generated sub-columns.  The driver's output is the mean over ims = 1..200."""
    nl = int(col["nlayers"])
    r2 = lambda v: np.asfortranarray(np.asarray(v, dtype=np.float64).reshape((1, nl)))
    al = None if alpha is None else r2(alpha)
    subs = []
    for ims in samples:
        g = mcica_subcol_lw(1, nl, int(col["icld"]), ims * gpoints(), irng, r2(col["pavel"]), r2(col["cldfrac"]), r2(col["ciwp"]),
                            r2(col["clwp"]), r2(col["rei"]), r2(col["rel"]),
                            np.asfortranarray(np.asarray(col["tauc"], dtype=np.float64).reshape((NBND, 1, nl), order="F")), al)
        subs.append(dict(cldfmc=g["cldfmcl"][:, 0, :], taucmc=g["taucmcl"][:, 0, :], ciwpmc=g["ciwpmcl"][:, 0, :],
                         clwpmc=g["clwpmcl"][:, 0, :], reicmc=g["reicmcl"][0], relqmc=g["relqmcl"][0]))
    return run_columns_mcica([col] * len(subs), subs), subs


def finalize(selected_only=False):
    """Release the device state of every library this process has loaded (the 140- and the 256-g-point build keep separate states:
    workspace, pinned staging, generator caches, streams); selected_only = True: only that of the library select_gpoints chose."""
    global _initialised
    if selected_only:
        if _lib is not None:
            _lib.rrtmg_lw_hip_finalize()
        return
    for h in _libs.values():
        h.rrtmg_lw_hip_finalize()
    _initialised = False


# ---------------------------------------------------------------------------------------------------
# Aggregation of small calls (include/rrtmg_lw_hip.h: rrtmg_lw_hip_queue_*)
# ---------------------------------------------------------------------------------------------------
class ChunkQueue:
    """Collects rrtmg_lw calls on small column chunks and solves them in one device pass:

        q = ChunkQueue(nlay, icld, idrv, inflglw, iceflglw, liqflglw)
        outs = [q.add(chunk_dict) for chunk_dict in chunks]       # dicts as for rrtmg_lw_from_dict
        q.flush()                                                  # fills every `outs[k]`

    One call of 64 columns costs ~0.5 ms of launch latency on the GPU; a thousand of them queued cost one pass over 64 000 columns."""

    def __init__(self, nlay, icld, idrv, inflglw, iceflglw, liqflglw):
        self.nlay, self.idrv = int(nlay), int(idrv)
        self._keep = []
        _check(lib().rrtmg_lw_hip_queue_begin(C.c_int(int(nlay)), C.c_int(int(icld)), C.c_int(int(idrv)), C.c_int(int(inflglw)),
                                              C.c_int(int(iceflglw)), C.c_int(int(liqflglw))))

    def add(self, d, out=None):
        ncol, nlay = int(d["ncol"]), self.nlay
        shp = dict(play=(ncol, nlay), plev=(ncol, nlay + 1), tlay=(ncol, nlay), tlev=(ncol, nlay + 1), tsfc=(ncol,), emis=(ncol, NBND),
                   taucld=(NBND, ncol, nlay), tauaer=(ncol, nlay, NBND))
        arrs = [_f(d[k], shp.get(k, (ncol, nlay))) for k in _GCM_ORDER + _CLD_ORDER]
        if out is None:
            out = _out_arrays(ncol, nlay, self.idrv)
        null = C.cast(None, _dp)
        args = [C.c_int(ncol), C.cast(None, C.POINTER(C.c_int))] + [_p(a) for a in arrs]
        args += [_p(out[k]) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")]
        args += [_p(out["duflx_dt"]) if self.idrv == 1 else null, _p(out["duflxc_dt"]) if self.idrv == 1 else null]
        _check(lib().rrtmg_lw_hip_queue_add(*args))
        self._keep.append((arrs, out))          # the library holds pointers until the flush
        return out

    def columns(self):
        return int(lib().rrtmg_lw_hip_queue_columns())

    def flush(self):
        try:
            _check(lib().rrtmg_lw_hip_queue_flush())
        finally:
            self._keep = []
