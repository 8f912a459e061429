"""The sample variance and the device-resident forms of the averaging McICA entries, without a GPU: what the header declares, what the
Python wrappers refuse before they touch the library, and the header's recurrence in numpy (`recurrence`, which the GPU tests compare
the library with bit for bit) against np.var."""
import os
import re

import numpy as np
import pytest

from rrtmg_lw_amd import api, arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAR = ("uflx_var", "dflx_var", "hr_var")


def recurrence(xs):
    """include/rrtmg_lw_hip.h, "The sample variance": (mean, var) of the samples xs[0], xs[1], ... - float64, every operation rounded
    on its own, in the header's order"""
    S = np.array(xs[0], dtype=np.float64)
    M = np.zeros_like(S)
    n = len(xs)
    for s in range(1, n):
        x = np.asarray(xs[s], dtype=np.float64)
        c = float(s + 1)
        S = S + x
        t = c * x
        t = t - S
        tt = t * t
        M = M + tt / (c * (c - 1.0))
    if n == 1:
        return S, M
    return S / float(n), M / float(n - 1)


@pytest.fixture
def no_library(monkeypatch):
    """any use of the C library fails the test"""
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(api, "lib", boom)


# ---- the header ---------------------------------------------------------------------------------------------------------------------------
def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_three_entries():
    h = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    decl = lambda name: _norm(re.search(r"int " + name + r"\((.*?)\);", h, re.S).group(1))
    mean, mean_dev = decl("rrtmg_lw_hip_run_mcica_samples"), decl("rrtmg_lw_hip_run_mcica_samples_device")
    # the host entry: the list of rrtmg_lw_hip_run_mcica_samples followed by the three variances
    assert decl("rrtmg_lw_hip_run_mcica_samples_var") == mean + ", double *uflx_var, double *dflx_var, double *hr_var"
    # the device entry: the view, the list of the device entry as void pointers, the variances, the stream
    assert mean_dev.endswith(", void *stream")
    as_void = re.sub(r"(const )?double \*", lambda m: (m.group(1) or "") + "void *", mean_dev[:-len(", void *stream")])
    assert decl("rrtmg_lw_hip_run_mcica_samples_device_view") == \
        "const rrtmg_lw_hip_array_view *view, " + as_void + ", void *uflx_var, void *dflx_var, void *hr_var, void *stream"
    assert decl("rrtmg_lw_hip_get_alpha_device_view") == \
        "const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int icld, int idcor, double decorr_con, " \
        "const void *dz, const void *lat, int juldat, const void *cldfrac, void *alpha, void *stream"
    # the host alpha entry is what it was
    assert decl("rrtmg_lw_hip_get_alpha") == "int ncol, int nlay, int icld, int idcor, double decorr_con, const double *dz, const double *lat, " \
                                             "int juldat, const double *cldfrac, double *alpha"
    assert "sqrt(var / nsamp)" in h and "M = M + (t * t) / (c * (c - 1))" in h


# ---- the wrappers -------------------------------------------------------------------------------------------------------------------------
class _Tensor:
    """what the device wrappers look at before they build the call; its address is never asked for"""
    def __init__(self, shape, dtype="float64", strides=None):
        import torch
        self.dtype = getattr(torch, dtype)
        self.shape = tuple(shape)
        if strides is None:                         # first index fastest
            strides, acc = [], 1
            for n in self.shape:
                strides.append(acc)
                acc *= n
        self._strides = tuple(strides)

    def stride(self):
        return self._strides

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return False

    def data_ptr(self):
        raise AssertionError("the library was touched")


def _call(ncol=8, nlay=12, dtype="float64", **replace):
    d = {"ncol": ncol, "nlay": nlay, "icld": 2, "idrv": 0, "inflglw": 2, "iceflglw": 3, "liqflglw": 1}
    names = api._GCM_ORDER + api._CLD_ORDER
    for k in names:
        d[k] = _Tensor(arrays.reference_shape(k, ncol, nlay), dtype)
    out = {k: _Tensor(arrays.reference_shape(k, ncol, nlay), dtype) for k in ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")}
    out.update(replace)
    return d, out


def test_samples_device_refuses_spectral_outputs(no_library):
    d, out = _call(uflxs=_Tensor((8, 13, 16)))
    with pytest.raises(ValueError, match="uflxs.*spectral"):
        api.rrtmg_lw_mcica_samples_device(d, out, 280, 4)


@pytest.mark.parametrize("name", VAR)
def test_samples_device_refuses_a_variance_of_one_sample(no_library, name):
    d, out = _call(**{name: _Tensor(arrays.reference_shape(name, 8, 12))})
    with pytest.raises(ValueError, match=name + " with nsamp = 1"):
        api.rrtmg_lw_mcica_samples_device(d, out, 280, 1)


def test_samples_device_refuses_tensors_that_are_not_the_form_s(no_library):
    # a variance of the wrong shape (hr_var has nlay rows), float32 tensors without the form, a tensor that is no view of a field ld wide
    d, out = _call(hr_var=_Tensor((8, 13)))
    with pytest.raises(ValueError, match="hr_var"):
        api.rrtmg_lw_mcica_samples_device(d, out, 280, 4)
    d, out = _call(dtype="float32")
    with pytest.raises(TypeError, match="float32"):
        api.rrtmg_lw_mcica_samples_device(d, out, 280, 4)
    d, out = _call(uflx_var=_Tensor((8, 13)))
    with pytest.raises(ValueError, match="strides"):
        api.rrtmg_lw_mcica_samples_device(d, out, 280, 4, ld=16)
    with pytest.raises(ValueError, match="ld=4 is smaller"):
        api.rrtmg_lw_mcica_samples_device(d, out, 280, 4, ld=4)


def test_host_wrapper_refuses_a_variance_of_one_sample(no_library):
    from rrtmg_lw_amd.synth import make_gcm_inputs
    d = make_gcm_inputs(8, 12, "cloudy")
    with pytest.raises(ValueError, match="var=True with nsamp = 1"):
        api.rrtmg_lw_mcica_subcol_from_dict(d, 280, 0, icld=2, var=True)
    with pytest.raises(ValueError, match="nsamp = 3.*float32"):
        api.rrtmg_lw_mcica_subcol_from_dict(d, 280, 0, icld=2, nsamp=3, var=True, dtype=np.float32)


def test_alpha_device_checks_its_tensors(no_library):
    d = {"ncol": 8, "nlay": 12, "dz": _Tensor((8, 12)), "lat": _Tensor((8,)), "cldfr": _Tensor((8, 12))}
    with pytest.raises(ValueError, match="alpha"):
        api.get_alpha_device(d, _Tensor((8, 13)), 5, 1, 2000.0, 100)
    with pytest.raises(TypeError, match="dz"):
        api.get_alpha_device(dict(d, dz=_Tensor((8, 12), "float32")), _Tensor((8, 12)), 5, 1, 2000.0, 100)


def test_arrays_know_the_new_names():
    f = arrays.ArrayForm(4, 0, 1)
    assert arrays.reference_shape("dz", 5, 7) == (5, 7) and arrays.reference_shape("lat", 5, 7) == (5,)
    assert [arrays.reference_shape(k, 5, 7) for k in VAR] == [(5, 8), (5, 8), (5, 7)]
    x = {"dz": np.arange(35.0).reshape(5, 7), "lat": np.arange(5.0), "hr_var": np.arange(35.0).reshape(5, 7)}
    y = arrays.from_reference(x, f)
    assert y["dz"].dtype == np.float32 and np.array_equal(y["dz"], x["dz"][:, ::-1]) and np.array_equal(y["lat"], x["lat"])
    back = arrays.to_reference(y, f)
    assert all(np.array_equal(back[k], x[k]) for k in x)
    assert arrays.field_strides("uflx_var", 5, 7, arrays.REFERENCE, 9) == (1, 9)


# ---- the recurrence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 16, 64])
def test_recurrence_is_the_unbiased_sample_variance(n):
    rng = np.random.default_rng(n)
    base = rng.uniform(50.0, 500.0, (40, 30))                  # fluxes in W m-2
    xs = [base + rng.normal(0.0, 5.0, base.shape) for _ in range(n)]
    mean, var = recurrence(xs)
    acc = xs[0].copy()
    for x in xs[1:]:
        acc = acc + x
    assert np.array_equal(mean, acc / float(n))                 # the mean of the entries without variance
    ref = np.var(np.stack(xs), axis=0, ddof=1)
    rel = float((np.abs(var - ref) / ref).max())
    print(f"n = {n}: max relative difference to np.var(ddof=1) {rel:.2e}")
    # t = c x - S cancels about |x| / sd = 100 to 1 here, each term of M then carries a relative error of a few 100 eps = 1e-13;
    # at n = 2 there is one term and nothing averages out
    assert (var >= 0.0).all() and rel <= 1e-11


def test_identical_samples_have_no_variance():
    x = np.random.default_rng(1).uniform(50.0, 500.0, (20, 10))
    for n in (2, 3, 64):
        mean, var = recurrence([x] * n)
        # two identical samples: S = 2 x and t = 2 x - S are exact.  More of them: rounding level - S carries at most (c - 1) roundings
        # of relative size u = 2^-53 and c x one, so |t| <= c^2 u x, a term of M is at most about c^2 u^2 x^2, their sum n^3 u^2 x^2 / 3
        # and the variance below (n u x)^2: 1.3e-23 for x = 500 and n = 64 (observed: 2e-25)
        bound = (n * 2.0 ** -53 * 500.0) ** 2
        assert (var == 0.0).all() if n == 2 else var.max() <= bound, (n, var.max())
        assert np.abs(mean - x).max() <= n * 2.0 ** -53 * 500.0
