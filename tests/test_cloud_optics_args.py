"""The cloud-optics entries without a GPU: both shipped libraries export the three symbols the header declares, and the Python wrappers
(api.cloud_optics, api.cloud_optics_device) refuse arrays of another dtype, shape or layout instead of converting them - before the
library is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from rrtmg_lw_amd import api, arrays
from rrtmg_lw_amd.synth import make_gcm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rrtmg_lw_hip_cloud_optics", "rrtmg_lw_hip_cloud_optics_device", "rrtmg_lw_hip_cloud_optics_device_view")
NCOL, NLAY = 6, 5


def test_both_libraries_export_the_entries():
    h = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(", h), n
    for path in (api.LIB_PATH, api.LIB_PATH_G256):
        assert os.path.exists(path), "build it with __graft_entry__.build()"
        lib = ctypes.CDLL(path)
        for n in NAMES:
            assert hasattr(lib, n), (path, n)


def test_header_argument_lists():
    h = open(os.path.join(ROOT, "include", "rrtmg_lw_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    host = norm(re.search(r"int rrtmg_lw_hip_cloud_optics\((.*?)\);", h, re.S).group(1))
    dev = norm(re.search(r"int rrtmg_lw_hip_cloud_optics_device\((.*?)\);", h, re.S).group(1))
    view = norm(re.search(r"int rrtmg_lw_hip_cloud_optics_device_view\((.*?)\);", h, re.S).group(1))
    assert host.startswith("int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw, const double *cldfr, const double *taucld,")
    assert host.endswith("const double *plev, const double *h2ovmr, double *taucloud, int *ncbands, double *secdiff")
    assert dev == host + ", void *stream"
    assert view == "const rrtmg_lw_hip_array_view *view, " + dev.replace("const double *", "const void *").replace("double *", "void *")


def _call():
    d = make_gcm_inputs(NCOL, NLAY, "cloudy")
    return {k: (np.array(v, order="F") if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def test_host_wrapper_refuses_instead_of_converting():
    d = _call()
    with pytest.raises(TypeError, match="cldfr"):
        api.cloud_optics(dict(d, cldfr=d["cldfr"].astype(np.float32)))
    with pytest.raises(TypeError, match="reice"):
        api.cloud_optics(dict(d, reice=d["reice"].tolist()))
    with pytest.raises(ValueError, match="shape"):
        api.cloud_optics(dict(d, taucld=np.moveaxis(d["taucld"], 0, 2)))
    with pytest.raises(ValueError, match="shape"):
        api.cloud_optics(dict(d, plev=d["plev"][:, :-1]))
    with pytest.raises(TypeError, match="h2ovmr"):
        api.cloud_optics(dict(d, h2ovmr=None))
    with pytest.raises(ValueError, match="unknown output"):
        api.cloud_optics(d, out={"tauc": None})
    with pytest.raises(ValueError, match="no output"):
        api.cloud_optics(d, out={"taucloud": None, "ncbands": None, "secdiff": None})
    with pytest.raises(ValueError, match="ncbands"):
        api.cloud_optics(d, out={"ncbands": np.zeros(NCOL, dtype=np.int64)})
    with pytest.raises(ValueError, match="taucloud"):
        api.cloud_optics(d, out={"taucloud": np.zeros((NCOL, NLAY, 16))})                   # C order
    with pytest.raises(ValueError, match="secdiff"):
        api.cloud_optics(d, out={"secdiff": np.zeros((NCOL, 16), dtype=np.float32, order="F")})


def test_device_wrapper_refuses_instead_of_converting():
    """(CPU tensors: every check is made before the library is touched)"""
    torch = pytest.importorskip("torch")
    d = _call()
    t = lambda a: torch.from_numpy(a)
    x = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    out = arrays.empty_like_form(("taucloud", "secdiff"), NCOL, NLAY, arrays.REFERENCE)
    out["ncbands"] = torch.zeros(NCOL, dtype=torch.int32)
    with pytest.raises(TypeError, match="cldfr"):
        api.cloud_optics_device(dict(x, cldfr=x["cldfr"].float()), out)
    with pytest.raises(ValueError, match="cicewp"):
        api.cloud_optics_device(dict(x, cicewp=x["cicewp"].contiguous()), out)             # C order: not the reference form's strides
    with pytest.raises(ValueError, match="taucld"):
        api.cloud_optics_device(dict(x, taucld=x["taucld"][:, :, :-1]), out)
    with pytest.raises(ValueError, match="missing"):
        api.cloud_optics_device({k: v for k, v in x.items() if k != "plev"}, out)
    with pytest.raises(TypeError, match="ncbands"):
        api.cloud_optics_device(x, dict(out, ncbands=torch.zeros(NCOL, dtype=torch.int64)))
    with pytest.raises(ValueError, match="ncbands"):
        api.cloud_optics_device(x, dict(out, ncbands=torch.zeros(NCOL + 1, dtype=torch.int32)))
    with pytest.raises(TypeError, match="secdiff"):
        api.cloud_optics_device(x, dict(out, secdiff=out["secdiff"].float()))
    with pytest.raises(ValueError, match="taucloud"):
        api.cloud_optics_device(x, dict(out, taucloud=torch.zeros(NCOL, NLAY, 16, dtype=torch.float64)))
    with pytest.raises(TypeError, match="float32"):
        api.cloud_optics_device(x, out, form=(4, 0, 0))
    with pytest.raises(ValueError, match="ld=3"):
        api.cloud_optics_device(x, out, ld=3)
    with pytest.raises(ValueError, match="unknown output"):
        api.cloud_optics_device(x, {"tauc": None})
    with pytest.raises(ValueError, match="no output"):
        api.cloud_optics_device(x, {})
