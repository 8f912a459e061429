"""dtype=np.float32 of the Python interface (rrtmg_lw_amd/api.py, the *_r4 entries of the C ABI) without a GPU: the argument reaches the
library's float32 entry, which refuses like the float64 one does on a machine without a device; what cannot be combined is a ValueError."""
import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs


def _f32(d):
    return {k: np.asfortranarray(v, dtype=np.float32) if isinstance(v, np.ndarray) else v for k, v in d.items()}


def test_float32_call_without_device_is_a_loud_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rrtmg_lw_amd import api
    d = _f32(make_gcm_inputs(8, 20, "cloudy"))
    with pytest.raises(api.RrtmgLwError, match="rrtmg_lw_hip_init has not been called"):
        api.rrtmg_lw_from_dict(d, dtype=np.float32)
    with pytest.raises(api.RrtmgLwError, match="has not been called"):
        api.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, dtype=np.float32)
    lev = np.ones((8, 21), dtype=np.float32, order="F")
    with pytest.raises(api.RrtmgLwError, match="has not been called"):
        api.adjust_tsfc(8, 20, lev, np.zeros(8, dtype=np.float32), lev, lev, lev, dtype=np.float32)


def test_float32_with_spectral_is_a_value_error():
    from rrtmg_lw_amd import api
    d = _f32(make_gcm_inputs(8, 20, "cloudy"))
    with pytest.raises(ValueError, match="spectral"):
        api.rrtmg_lw_from_dict(d, dtype=np.float32, spectral=True)
    with pytest.raises(ValueError, match="spectral"):
        api.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, dtype=np.float32, spectral=True)
    with pytest.raises(ValueError, match="dtype"):
        api.rrtmg_lw_from_dict(d, dtype=np.float16)


def test_float32_outputs_are_checked_for_the_dtype_asked_for():
    from rrtmg_lw_amd import api
    d = _f32(make_gcm_inputs(8, 20, "cloudy"))
    out = api._out_arrays(8, 20, 0)                       # float64 arrays handed to a float32 call
    with pytest.raises(ValueError, match="float32"):
        api.rrtmg_lw_from_dict(d, out=out, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in api._out_arrays(8, 20, 1, np.float32).values())
