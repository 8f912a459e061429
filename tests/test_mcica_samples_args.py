"""The mean over several sub-column samples, without a GPU: what the Python wrappers refuse before they touch the library, and what the
header declares."""
import os
import re

import numpy as np
import pytest

from rrtmg_lw_amd import api
from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any use of the C library fails the test"""
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(api, "lib", boom)


class _Tensor:
    """what the device wrapper looks at before it builds the call: a dtype"""
    def __init__(self, dtype):
        self.dtype = dtype

    def data_ptr(self):
        raise AssertionError("the library was touched")


@pytest.mark.parametrize("kw,text", [({"spectral": True}, "spectral"), ({"dtype": np.float32}, "float32")])
def test_host_wrapper_refuses_what_the_entry_does_not_offer(no_library, kw, text):
    d = make_gcm_inputs(8, 12, "cloudy")
    with pytest.raises(ValueError, match="nsamp = 3.*" + text):
        api.rrtmg_lw_mcica_subcol_from_dict(d, 280, 0, icld=2, nsamp=3, **kw)
    with pytest.raises(ValueError, match="nsamp = 3.*" + text):
        api.rrtmg_lw_mcica_subcol(8, 12, 2, 0, 280, 0, *[d[k] for k in api._GCM_ORDER], d["inflglw"], d["iceflglw"], d["liqflglw"],
                                  d["cldfr"], d["taucld"], d["cicewp"], d["cliqwp"], d["reice"], d["reliq"], None, d["tauaer"], nsamp=3, seedstep=140, **kw)


@pytest.mark.parametrize("kw,dtype,spec,text", [
    ({"form": (4, 0, 0)}, "torch.float64", False, "form="),
    ({"ld": 16}, "torch.float64", False, "ld="),
    ({}, "torch.float64", True, "spectral"),
    ({}, "torch.float32", False, "float32"),
])
def test_device_wrapper_refuses_what_the_entry_does_not_offer(no_library, kw, dtype, spec, text):
    d = {"ncol": 8, "nlay": 12, "icld": 2, "idrv": 0}
    out = {"uflx": _Tensor(dtype)}
    if spec:
        out["uflxs"] = _Tensor(dtype)
    with pytest.raises(ValueError, match="nsamp = 2.*" + text):
        api.rrtmg_lw_mcica_subcol_device(d, out, 280, 0, nsamp=2, **kw)


def test_header_declares_the_entries_and_the_constant():
    h = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    m = re.search(r"#define\s+RRTMG_LW_HIP_MAX_SAMPLES\s+(\d+)", h)
    assert m and int(m.group(1)) >= 1
    for name, tail in (("rrtmg_lw_hip_run_mcica_samples", r"double \*duflxc_dt\);"), ("rrtmg_lw_hip_run_mcica_samples_device", r"double \*duflxc_dt, void \*stream\);")):
        decl = re.search(r"int " + name + r"\(\s*int ncol, int nlay, int \*icld, int idrv, int permuteseed, int nsamp, int seedstep, int \*irng,(.*?);", h, re.S)
        assert decl, name
        assert re.search(tail, decl.group(0)), name
    assert re.search(r"long long rrtmg_lw_hip_kiss_tables_built\(void\);", h)
    # the argument list is the fused entry's with the two integers behind permuteseed
    fused = re.search(r"int rrtmg_lw_hip_run_mcica_subcol\((.*?)\);", h, re.S).group(1)
    mean = re.search(r"int rrtmg_lw_hip_run_mcica_samples\((.*?)\);", h, re.S).group(1)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(mean) == norm(fused.replace("int permuteseed,", "int permuteseed, int nsamp, int seedstep,"))
