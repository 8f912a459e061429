"""What the C entries refuse, and how: every call here is one tiny call (4 columns, 6 layers) or a refusal the driver makes before it
stages anything - no case hands the library a null it would read or write through.

Raw ctypes on the library (rrtmg_lw_amd.api checks shapes itself and never passes a null where the interface wants an array):

 a. the valid call returns 0;
 b. with icld = 2, a null in place of each required input in turn returns RRTMG_LW_HIP_EARG and rrtmg_lw_hip_last_error names a null
    array; for play .. emis and tauaer the text carries a position ("argument N"), the array's 0-based place in rrtmg_lw's list of
    arrays - play 0 .. emis 15, the six cloud arrays 16 .. 21, tauaer 22 - on every entry (the fused entry's optional alpha is no
    required input; its generator refuses a null play or cldfr itself, without a position);
 c. with icld = 0 the non-McICA entries and the queue accept null cloud arrays;
 d. a null in place of each required output returns EARG;
 e. idrv = 1 with a null duflx_dt returns EARG and says "idrv=1 needs";
 f. icld = 9 comes back as 2 from the non-McICA and the McICA entries;
 g. a call this small goes through the combining entry (rrtmg_lw_hip_combine_stats counts it), whose refusals are those of the entry
    that takes the lock.

Not covered, because the driver does not make these checks (the cases would hand it a null to work with): null broadband outputs on
rrtmg_lw_hip_run_mcica[_spectral] and on every device-pointer entry, null inputs on the device-pointer entries."""
import ctypes as C
import re

import numpy as np
import pytest

from rrtmg_lw_amd.synth import make_gcm_inputs

pytestmark = pytest.mark.gpu

NCOL, NLAY = 4, 6
EARG = 2
GCM = ("play", "plev", "tlay", "tlev", "tsfc", "h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr",
       "ccl4vmr", "emis")
CLD = ("cldfr", "taucld", "cicewp", "cliqwp", "reice", "reliq")
MC = ("cldfmcl", "taucmcl", "ciwpmcl", "clwpmcl", "reicmcl", "relqmcl")
OUT6 = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
OUT8 = OUT6 + ("duflx_dt", "duflxc_dt")
SPEC = ("uflxs", "dflxs", "uflxcs", "dflxcs")
OPT = ("taug", "fracs", "planklay", "planklev", "plankbnd", "dplankbnd_dt")
# the array's place in rrtmg_lw's list (the McICA entries take their sub-column arrays where rrtmg_lw takes the cloud arrays)
PLACE = {k: i for i, k in enumerate(GCM + CLD + ("tauaer",))}
PLACE.update({k: 16 + i for i, k in enumerate(MC)})

HOST_GCM = ("run_nomcica", "run_nomcica_spectral", "run_mcica", "run_mcica_spectral", "run_mcica_subcol", "run_mcica_subcol_spectral")
DEVICE_GCM = tuple(e + "_device" for e in HOST_GCM)


def _inputs_of(entry):
    return GCM + (MC if entry.startswith("run_mcica") and "subcol" not in entry else CLD) + ("tauaer",)


def _arrays():
    """host arrays of every entry: the synthetic cloudy inputs, sub-column arrays of the same clouds, every output"""
    d = make_gcm_inputs(NCOL, NLAY, "cloudy")
    ng = 140
    a = {k: np.asfortranarray(d[k], dtype=np.float64) for k in GCM + CLD + ("tauaer",)}
    on = (a["cldfr"] > 0.5).astype(np.float64)
    a["cldfmcl"] = np.asfortranarray(np.broadcast_to(on, (ng, NCOL, NLAY)))
    a["ciwpmcl"] = np.asfortranarray(a["cldfmcl"] * a["cicewp"])
    a["clwpmcl"] = np.asfortranarray(a["cldfmcl"] * a["cliqwp"])
    a["taucmcl"] = np.zeros((ng, NCOL, NLAY), order="F")
    a["reicmcl"], a["relqmcl"] = a["reice"].copy(order="F"), a["reliq"].copy(order="F")
    for k in OUT8:
        a[k] = np.zeros((NCOL, NLAY if k in ("hr", "hrc") else NLAY + 1), order="F")
    for k in SPEC:
        a[k] = np.zeros((NCOL, NLAY + 1, 16), order="F")
    for k, shape in dict(taug=(NCOL, NLAY, ng), fracs=(NCOL, NLAY, ng), planklay=(NCOL, NLAY, 16), planklev=(NCOL, NLAY + 1, 16),
                         plankbnd=(NCOL, 16), dplankbnd_dt=(NCOL, 16)).items():
        a[k] = np.zeros(shape, order="F")
    return a, (int(d["inflglw"]), int(d["iceflglw"]), int(d["liqflglw"]))


def _device_arrays():
    import torch
    dev = torch.device("cuda", 0)
    d = make_gcm_inputs(NCOL, NLAY, "cloudy", backend="torch", device=dev)
    a = {k: d[k] for k in GCM + CLD + ("tauaer",)}
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    for k in MC:
        a[k] = z(NLAY, NCOL) + (30.0 if k == "reicmcl" else 10.0) if k in ("reicmcl", "relqmcl") else z(NLAY, NCOL, 140)
    for k in OUT8:
        a[k] = z(NLAY if k in ("hr", "hrc") else NLAY + 1, NCOL)
    for k in SPEC:
        a[k] = z(16, NLAY + 1, NCOL)
    a.update(taug=z(140, NLAY, NCOL), fracs=z(140, NLAY, NCOL), planklay=z(16, NLAY, NCOL), planklev=z(16, NLAY + 1, NCOL),
             plankbnd=z(16, NCOL), dplankbnd_dt=z(16, NCOL))
    return a, (int(d["inflglw"]), int(d["iceflglw"]), int(d["liqflglw"]))


class _Caller:
    """Builds the C argument list of an entry from named arrays; `null` names the arrays to pass as null pointers."""

    def __init__(self, hip, arrays, flags, device=False):
        self.hip, self.lib, self.a, self.flags, self.device = hip, hip.lib(), arrays, flags, device

    def ptr(self, name, null):
        if name in null:
            return C.c_void_p(0)
        return C.c_void_p(self.a[name].data_ptr() if self.device else self.a[name].ctypes.data)

    def err(self):
        return self.lib.rrtmg_lw_hip_last_error().decode()

    def gcm(self, entry, icld=2, idrv=0, null=(), irng=0):
        """one of HOST_GCM / DEVICE_GCM; returns (rc, icld as it comes back)"""
        ic, rng = C.c_int(icld), C.c_int(irng)
        args = [C.c_int(NCOL), C.c_int(NLAY), C.byref(ic), C.c_int(idrv)]
        if "subcol" in entry:
            args += [C.c_int(7), C.byref(rng)]
        args += [self.ptr(k, null) for k in GCM] + [C.c_int(f) for f in self.flags]
        args += [self.ptr(k, null) for k in _inputs_of(entry)[16:22]]
        if "subcol" in entry:
            args.append(C.c_void_p(0))                      # alpha: optional (icld = 4 / 5 only)
        args.append(self.ptr("tauaer", null))
        no_dt = () if idrv == 1 else ("duflx_dt", "duflxc_dt")
        args += [self.ptr(k, tuple(null) + no_dt) for k in OUT8]
        if "spectral" in entry:
            args += [self.ptr(k, null) for k in SPEC]
        if self.device:
            args.append(C.c_void_p(0))
        rc = getattr(self.lib, "rrtmg_lw_hip_" + entry)(*args)
        if self.device:
            self.hip.check(None)
        return rc, ic.value

    def queue_add(self, null=(), idrv=0):
        no_dt = () if idrv == 1 else ("duflx_dt", "duflxc_dt")
        args = [C.c_int(NCOL), C.c_void_p(0)] + [self.ptr(k, null) for k in GCM + CLD + ("tauaer",)]
        args += [self.ptr(k, tuple(null) + no_dt) for k in OUT8]
        return self.lib.rrtmg_lw_hip_queue_add(*args)

    def queue_begin(self, icld=2, idrv=0):
        return self.lib.rrtmg_lw_hip_queue_begin(C.c_int(NLAY), C.c_int(icld), C.c_int(idrv), *[C.c_int(f) for f in self.flags])

    def optics(self, idrv=0, null=()):
        no_dt = () if idrv == 1 else ("dplankbnd_dt",)
        args = [C.c_int(NCOL), C.c_int(NLAY), C.c_int(idrv)] + [self.ptr(k, null) for k in GCM] + [self.ptr(k, tuple(null) + no_dt) for k in OPT]
        if self.device:
            rc = self.lib.rrtmg_lw_hip_gas_optics_device(*args, C.c_void_p(0))
            self.hip.check(None)
            return rc
        return self.lib.rrtmg_lw_hip_gas_optics(*args)


@pytest.fixture(scope="module")
def host(hip):
    return _Caller(hip, *_arrays())


@pytest.fixture(scope="module")
def device(hip):
    return _Caller(hip, *_device_arrays(), device=True)


def _names_null_input(text, name, generator=False):
    """The refusal names a null array.  For play .. emis and tauaer it gives the array's place in rrtmg_lw's list; the cloud arrays'
    refusal carries no position unless the entry is the queue, and the fused entries' generator refuses its own inputs (play, cldfr)
    first, by name of the generator."""
    assert "null" in text, text
    if generator and name in ("play", "cldfr"):
        assert text == "null generator input", (name, text)
        return
    m = re.search(r"argument (\d+)", text)
    if m or name not in CLD + MC:
        assert m and int(m.group(1)) == PLACE[name], (name, text)


# ---- a, f: valid calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", HOST_GCM)
def test_valid_host_call(host, entry):
    assert host.gcm(entry) == (0, 2), host.err()
    assert host.gcm(entry, idrv=1) == (0, 2), host.err()
    assert np.isfinite(host.a["uflx"]).all() and host.a["uflx"].min() > 0.0


def test_valid_queue_and_gas_optics(host):
    assert host.queue_begin() == 0, host.err()
    assert host.queue_add() == 0, host.err()
    assert host.lib.rrtmg_lw_hip_queue_flush() == 0, host.err()
    assert host.optics() == 0, host.err()
    assert host.optics(idrv=1) == 0, host.err()


@pytest.mark.parametrize("entry", ("run_nomcica", "run_nomcica_spectral", "run_mcica", "run_mcica_spectral"))
def test_icld_out_of_range_comes_back_as_2(host, device, entry):
    assert host.gcm(entry, icld=9) == (0, 2), host.err()
    assert device.gcm(entry + "_device", icld=9) == (0, 2), device.err()


# ---- b: null inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", HOST_GCM)
def test_null_input_is_refused(host, entry):
    for name in _inputs_of(entry):
        rc, _ = host.gcm(entry, null=(name,))
        assert rc == EARG, (name, rc, host.err())
        _names_null_input(host.err(), name, generator="subcol" in entry)


def test_null_input_is_refused_by_the_queue(host):
    assert host.queue_begin() == 0, host.err()
    for name in GCM + CLD + ("tauaer",):
        assert host.queue_add(null=(name,)) == EARG, name
        _names_null_input(host.err(), name)
        assert re.search(r"argument (\d+)", host.err())          # (the queue names the position of every array)
    assert host.lib.rrtmg_lw_hip_queue_columns() == 0
    assert host.lib.rrtmg_lw_hip_queue_flush() == 0


def test_null_input_is_refused_by_gas_optics(host):
    for name in GCM:
        assert host.optics(null=(name,)) == EARG, name
        _names_null_input(host.err(), name)


# ---- c: icld = 0 does not read the cloud arrays -------------------------------------------------------------------------------------------
def test_clear_sky_accepts_null_cloud_arrays(host):
    for entry in ("run_nomcica", "run_nomcica_spectral"):
        assert host.gcm(entry, icld=0, null=CLD) == (0, 0), host.err()
    assert host.queue_begin(icld=0) == 0, host.err()
    assert host.queue_add(null=CLD) == 0, host.err()
    assert host.lib.rrtmg_lw_hip_queue_flush() == 0, host.err()


# ---- d: null outputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", HOST_GCM)
def test_null_output_is_refused(host, entry):
    # (rrtmg_lw_hip_run_mcica[_spectral] do not check their broadband outputs: see the module's docstring)
    names = (() if entry.startswith("run_mcica") and "subcol" not in entry else OUT6) + (SPEC[:2] if "spectral" in entry else ())
    for name in names:
        rc, _ = host.gcm(entry, null=(name,))
        assert rc == EARG, (name, rc, host.err())
        assert ("null output" in host.err()) if name in OUT6 else ("uflxs and dflxs are required" in host.err()), host.err()


def test_null_output_is_refused_by_the_queue_and_gas_optics(host):
    assert host.queue_begin() == 0, host.err()
    for name in OUT6:
        assert host.queue_add(null=(name,)) == EARG, name
        assert "null output" in host.err()
    for name in ("taug", "fracs"):
        assert host.optics(null=(name,)) == EARG, name
        assert "taug and fracs are required" in host.err()


@pytest.mark.parametrize("entry", [e for e in DEVICE_GCM if "spectral" in e])
def test_null_spectral_output_is_refused_by_the_device_entries(device, entry):
    for name in SPEC[:2]:
        rc, _ = device.gcm(entry, null=(name,))
        assert rc == EARG and "uflxs and dflxs are required" in device.err(), (name, rc, device.err())


def test_null_output_is_refused_by_device_gas_optics(device):
    assert device.optics() == 0, device.err()
    for name in ("taug", "fracs"):
        assert device.optics(null=(name,)) == EARG and "taug and fracs are required" in device.err(), name


# ---- e: idrv = 1 needs the derivative outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", HOST_GCM + DEVICE_GCM)
def test_idrv_1_needs_the_derivative_outputs(host, device, entry):
    who = device if entry.endswith("_device") else host
    for name in ("duflx_dt", "duflxc_dt"):
        rc, _ = who.gcm(entry, idrv=1, null=(name,))
        assert rc == EARG and "idrv=1 needs" in who.err(), (name, rc, who.err())


def test_idrv_1_needs_the_derivative_outputs_queue_and_gas_optics(host, device):
    assert host.queue_begin(idrv=1) == 0, host.err()
    for name in ("duflx_dt", "duflxc_dt"):
        assert host.queue_add(null=(name,), idrv=1) == EARG and "idrv=1 needs" in host.err(), name
    assert host.queue_begin() == 0, host.err()
    for who in (host, device):
        assert who.optics(idrv=1, null=("dplankbnd_dt",)) == EARG and "idrv=1 needs" in who.err()


# ---- g: the combining entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("run_nomcica", "run_mcica_subcol"))
def test_small_call_goes_through_the_combining_entry(host, entry):
    calls0, _ = host.hip.combine_stats()
    assert host.gcm(entry) == (0, 2), host.err()
    assert host.hip.combine_stats()[0] == calls0 + 1
    # the combining entry's refusals are those of the entry that takes the lock (the spectral twin never combines)
    for name in _inputs_of(entry) + OUT6:
        assert host.gcm(entry, null=(name,))[0] == EARG, name
        mine = host.err()
        assert host.gcm(entry + "_spectral", null=(name,))[0] == EARG, name
        assert host.err() == mine, name
    for name in ("duflx_dt", "duflxc_dt"):
        assert host.gcm(entry, idrv=1, null=(name,))[0] == EARG, name
        assert "idrv=1 needs" in host.err()
