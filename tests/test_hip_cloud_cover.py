"""rrtmg_lw_hip_mcica_cloud_cover, _device and _device_view (include/rrtmg_lw_hip.h, "Cloud cover as the McICA sub-columns realise it"):
total cover, cumulative and per-layer cover and the packed sub-column mask, counted from the mask the fused McICA entries draw.

Every comparison is exact (array_equal): the expected values are numpy applied to the reference generator's own cldfmcl
(Oracle.mcica_subcol; tests/cloud_cover_ref.py holds the definitions and the designed cloud fields) - integer counts and one float64
division, which any implementation reproduces bit for bit.  131 columns (two 64-column blocks and a ragged tail) x 13 layers; the
generator runs once for all columns of a call, so there are no column batches to cross - set_batch is exercised all the same."""
import ctypes as C

import numpy as np
import pytest

import cloud_cover_ref as ccr
from cloud_cover_ref import NCOL, NLAY
from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.arrays import REFERENCE, ArrayForm

from test_hip_device_views import _check_outputs, _dev, _embed_inputs, _host, _output_fields, _stream, fid  # noqa: E402
from test_g256 import hip256  # noqa: E402,F401  (the fixture that selects the 256-g-point library for one test)

gpu = pytest.mark.gpu

SEED, DECORR, JULDAT = 421, 2500.0, 100
FLOATS = ("cldtot", "cldcum", "cldlay")
ALL = FLOATS + ("submask",)
R4, R8TOP, R4LFTOP = ArrayForm(4, 0, 0), ArrayForm(8, 0, 1), ArrayForm(4, 1, 1)
PAD, C0 = 7, 3                # fields ncol + 7 wide, the call's columns from column 3
MASK_FILL = -0x21524111       # (int32; no mask word of the tests has this pattern)
EARG = 2


# ---- the numpy helper itself, and the designed fields (no GPU) ---------------------------------------------------------------------------
def test_helper_on_a_hand_written_mask():
    """3 sub-columns, 2 columns, 4 layers (index 0 at the surface)"""
    c = np.zeros((3, 2, 4))
    c[0, 0, 1] = 1                         # column 0: sub-column 0 cloudy in layer 1,
    c[1, 0, 1] = c[1, 0, 3] = 1            #           sub-column 1 in layers 1 and 3, sub-column 2 clear
    c[:, 1, 2] = 1                         # column 1: overcast layer 2
    lay, cum = ccr.counts(c)
    assert lay.tolist() == [[0, 2, 0, 1], [0, 0, 3, 0]]
    assert cum.tolist() == [[2, 2, 1, 1], [3, 3, 3, 0]]
    r = ccr.cover([c])
    assert r["cldtot"].tolist() == [2 / 3, 1.0]
    assert r["cldcum"].tolist() == [[2 / 3, 2 / 3, 1 / 3, 1 / 3], [1.0, 1.0, 1.0, 0.0]]
    assert r["cldlay"].tolist() == [[0.0, 2 / 3, 0.0, 1 / 3], [0.0, 0.0, 1.0, 0.0]]
    # two samples: counts add, one division by 6
    c2 = np.zeros((3, 2, 4))
    c2[2, 0, 0] = 1
    r2 = ccr.cover([c, c2])
    assert r2["cldtot"].tolist() == [3 / 6, 3 / 6] and r2["cldcum"][0].tolist() == [3 / 6, 2 / 6, 1 / 6, 1 / 6]
    assert r2["cldlay"][0].tolist() == [1 / 6, 2 / 6, 0.0, 1 / 6]
    # float32: the float64 quotient rounded once
    assert ccr.cover([c], np.float32)["cldtot"][0] == np.float32(2 / 3) and ccr.cover([c], np.float32)["cldtot"].dtype == np.float32
    # the packed mask: 70 sub-columns -> 3 words, bits past sub-column 69 stay zero
    big = np.zeros((70, 1, 2))
    big[[0, 31, 32, 69], 0, 0] = 1
    big[:, 0, 1] = 1
    m = ccr.submask(big)
    assert m.shape == (1, 2, 3) and m.dtype == np.uint32
    assert m[0, 0].tolist() == [0x80000001, 0x1, 1 << 5] and m[0, 1].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, (1 << 6) - 1]
    with pytest.raises(AssertionError):
        ccr.counts(np.full((3, 2, 4), 0.5))


_IN, _CLD = {}, {}


def _inputs(oracle, icld, form=REFERENCE):
    """Once per (overlap family, form): the designed inputs as `form` stores them (numpy; a float32 form rounds 0.3), alpha among them -
    the oracle's get_alpha of the widened inputs, rounded as the form stores it - and the same widened to the float64 reference form,
    which is what the generator sees.  Shared by the tests and left unchanged."""
    form = ArrayForm(*form)
    key = (icld if icld in (4, 5) else 0, tuple(form))
    if key not in _IN:
        g = ccr.designed_inputs()
        x = arrays.from_reference({k: g[k] for k in ("play", "cldfr", "dz")}, form)
        w = arrays.to_reference(x, form)
        if icld in (4, 5):
            a = oracle.get_alpha(NCOL, NLAY, icld, 0, DECORR, w["dz"], g["lat"], JULDAT, w["cldfr"])
            x.update(arrays.from_reference({"alpha": a}, form))
            w = arrays.to_reference(x, form)
            assert w["alpha"].max() > 0.1
        for v in list(x.values()) + list(w.values()):
            v.setflags(write=False)
        _IN[key] = (dict(x, ncol=NCOL, nlay=NLAY), w)
    return _IN[key]


def _cldfmcl(oracle, icld, irng, seed, form=REFERENCE, gpoints=140):
    """Once per key: the reference generator's cldfmcl for the designed inputs of `form`"""
    key = (icld, irng, seed, tuple(form), gpoints)
    if key not in _CLD:
        if gpoints != 140:
            from oracle.bindings import Oracle
            oracle = Oracle(gpoints=gpoints)
        _, w = _inputs(oracle, icld, form)
        c = ccr.oracle_cldfmcl(oracle, icld, seed, irng, w["play"], w["cldfr"], w.get("alpha"))
        assert c.shape == (gpoints, NCOL, NLAY)
        c.setflags(write=False)
        _CLD[key] = c
    return _CLD[key]


@pytest.mark.parametrize("icld", [1, 2, 3, 4, 5])
def test_designed_fields_give_partial_cover_for_every_overlap(oracle, icld):
    """oracle only: the fields exercise what they are designed for, whatever the overlap rule"""
    g = ccr.designed_inputs()
    assert (g["cldfr"] == 1.0).any() and (g["cldfr"] == 1e-21).any() and (g["cldfr"].max(axis=1) == 0).any()
    assert (g["cldfr"][:, 0] > 0).any() and (g["cldfr"][:, -1] > 0).any()
    for irng in (0, 1):
        r = ccr.cover([_cldfmcl(oracle, icld, irng, SEED)])
        tot = r["cldtot"]
        assert ((tot > 0) & (tot < 1)).any() and (tot == 0).any() and (tot == 1).any()
        assert np.array_equal(r["cldcum"][:, 0], tot) and (np.diff(r["cldcum"], axis=1) <= 0).all()
        only_tiny = (g["cldfr"].max(axis=1) == 1e-21)
        assert only_tiny.any() and (tot[only_tiny] == 0).all()                   # 1e-21 is below cldmin: clear
        m = ccr.submask(_cldfmcl(oracle, icld, irng, SEED))
        assert (m[:, :, 4] >> 12 == 0).all() and (m[g["cldfr"] == 1.0] == [0xFFFFFFFF] * 4 + [0xFFF]).all()


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------
def _want(oracle, icld, irng, form=REFERENCE, nsamp=1, step=140, gpoints=140):
    """the four outputs in the float64 / float32 reference layout"""
    cs = [_cldfmcl(oracle, icld, irng, SEED + s * step, form, gpoints) for s in range(nsamp)]
    w = ccr.cover(cs, np.float64 if ArrayForm(*form).real_bytes == 8 else np.float32)
    if nsamp == 1:
        w["submask"] = ccr.submask(cs[0])
    return w


def _mask_tensor(mw, fill=MASK_FILL):
    import torch
    return torch.full((mw, NLAY, NCOL), fill, dtype=torch.int32, device="cuda:0").permute(2, 1, 0)


def _plain_device(hip, oracle, icld, irng, names=ALL, nsamp=1, step=None):
    """rrtmg_lw_hip_mcica_cloud_cover_device on contiguous reference-form tensors -> the outputs as numpy arrays"""
    x, _ = _inputs(oracle, icld)
    xd = _dev({k: v for k, v in x.items() if k != "dz"})
    out = arrays.empty_like_form([k for k in names if k != "submask"], NCOL, NLAY, REFERENCE, device="cuda:0", fill=float("nan"))
    if "submask" in names:
        out["submask"] = _mask_tensor(hip.mask_words())
    s = _stream()
    r = hip.mcica_cloud_cover_device(xd, out, icld, SEED, irng=irng, alpha=xd.get("alpha"), nsamp=nsamp, seedstep=step, stream=s)
    hip.check(s)
    assert r == irng
    got = _host(out)
    if "submask" in got:
        got["submask"] = got["submask"].view(np.uint32)
    return got


def _assert_equal(got, want, names):
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@gpu
@pytest.mark.parametrize("irng", [0, 1])
@pytest.mark.parametrize("icld", [1, 2, 3, 4, 5])
def test_counts_equal_the_oracles_subcolumns(hip, oracle, icld, irng):
    x, w = _inputs(oracle, icld)
    want = _want(oracle, icld, irng)
    got = hip.mcica_cloud_cover(NCOL, NLAY, icld, SEED, irng, w["play"], w["cldfr"], alpha=w.get("alpha"), outputs=ALL)
    assert got["irng"] == irng
    _assert_equal(got, want, ALL)
    assert np.array_equal(got["cldcum"][:, 0], got["cldtot"])
    ng = hip.gpoints()
    assert got["submask"].shape == (NCOL, NLAY, 5) and (got["submask"][:, :, -1] >> np.uint32(ng % 32) == 0).all()
    assert ((got["cldtot"] > 0) & (got["cldtot"] < 1)).any()
    _assert_equal(_plain_device(hip, oracle, icld, irng), want, ALL)


@gpu
def test_outputs_are_optional_each_on_its_own(hip, oracle):
    want = _want(oracle, 2, 0)
    for names in (("cldtot",), ("cldcum",), ("cldlay",), ("submask",), ("cldtot", "submask")):
        _assert_equal(_plain_device(hip, oracle, 2, 0, names=names), want, names)
        x, w = _inputs(oracle, 2)
        got = hip.mcica_cloud_cover(NCOL, NLAY, 2, SEED, 0, w["play"], w["cldfr"], outputs=names)
        assert set(got) == set(names) | {"irng"}
        _assert_equal(got, want, names)


@gpu
@pytest.mark.parametrize("icld", [2, 4])
def test_three_samples_add_their_counts(hip, oracle, icld):
    ng = hip.gpoints()
    x, w = _inputs(oracle, icld)
    want = _want(oracle, icld, 0, nsamp=3, step=ng)
    one = _want(oracle, icld, 0)
    assert not np.array_equal(want["cldtot"], one["cldtot"])                    # (a mean over different samples, not sample 0)
    got = hip.mcica_cloud_cover(NCOL, NLAY, icld, SEED, 0, w["play"], w["cldfr"], alpha=w.get("alpha"), nsamp=3, seedstep=ng)
    _assert_equal(got, want, FLOATS)
    assert np.array_equal(got["cldcum"][:, 0], got["cldtot"])
    _assert_equal(_plain_device(hip, oracle, icld, 0, names=FLOATS, nsamp=3, step=ng), want, FLOATS)
    # one sample, whatever the step: the single call
    _assert_equal(_plain_device(hip, oracle, icld, 0, nsamp=1, step=ng), one, ALL)
    _assert_equal(_plain_device(hip, oracle, icld, 0, nsamp=1, step=7), one, ALL)
    # another step draws other samples
    other = ccr.cover([_cldfmcl(oracle, icld, 0, SEED + s * 7) for s in range(3)])
    _assert_equal(_plain_device(hip, oracle, icld, 0, names=FLOATS, nsamp=3, step=7), other, FLOATS)


def _view_call(hip, oracle, form, wide, icld, irng, nsamp=1):
    """rrtmg_lw_hip_mcica_cloud_cover_device_view on views of fields NCOL + PAD wide (or on contiguous tensors of the form): checks the
    results against the oracle's for the inputs as the form stores them, and that nothing else in the fields was written"""
    import torch
    form = ArrayForm(*form)
    x, _ = _inputs(oracle, icld, form)
    ld, c0 = (NCOL + PAD, C0) if wide else (0, 0)
    width = ld or NCOL
    xin = _embed_inputs(x, form, width, c0, ("play", "cldfr", "alpha"))
    fields, views = _output_fields(FLOATS, NCOL, NLAY, form, width, c0)
    mw, guard = hip.mask_words(), 64
    buf = None
    if nsamp == 1:
        # submask: int32 words behind and in front of which - and in whose other columns - the fill must survive
        buf = torch.full((guard + mw * NLAY * width + guard,), MASK_FILL, dtype=torch.int32, device="cuda:0")
        if form.layer_fastest:
            views["submask"] = buf[guard:guard + NCOL * NLAY * mw].view(NCOL, NLAY, mw)
        else:
            views["submask"] = buf[guard + c0:].as_strided((NCOL, NLAY, mw), (1, width, width * NLAY))
    s = _stream()
    ng = hip.gpoints()
    r = hip.mcica_cloud_cover_device(dict(x, **xin), views, icld, SEED, irng=irng, alpha=xin.get("alpha"), nsamp=nsamp, seedstep=ng, stream=s,
                                     form=None if form == REFERENCE else form, ld=ld)
    hip.check(s)
    assert r == irng
    want = _want(oracle, icld, irng, form, nsamp, ng)
    wf = arrays.from_reference({k: want[k] for k in FLOATS}, form)
    _check_outputs(fields, {k: views[k] for k in FLOATS}, wf, FLOATS, form, NCOL, c0)
    if buf is not None:
        m = want["submask"][:, ::-1, :] if form.top_first else want["submask"]
        expect = np.full(buf.shape, MASK_FILL, dtype=np.int32)
        if form.layer_fastest:
            expect[guard:guard + NCOL * NLAY * mw] = np.ascontiguousarray(m).view(np.int32).ravel()
        else:
            np.lib.stride_tricks.as_strided(expect[guard + c0:], (NCOL, NLAY, mw), (4, 4 * width, 4 * width * NLAY))[...] = m.view(np.int32)
        assert np.array_equal(buf.cpu().numpy(), expect), "submask: wrong words, or words outside the call's columns written"
    return {k: v.cpu().numpy() for k, v in views.items()}


FORMS = [(REFERENCE, True), (R4, True), (R8TOP, True), (R4LFTOP, False)]


@gpu
@pytest.mark.parametrize("icld,irng,nsamp", [(2, 0, 1), (5, 1, 1), (4, 0, 3)])
@pytest.mark.parametrize("form,wide", FORMS, ids=lambda v: fid(v) if isinstance(v, tuple) else "")
def test_every_form_and_a_wider_field(hip, oracle, form, wide, icld, irng, nsamp):
    _view_call(hip, oracle, form, wide, icld, irng, nsamp)


@gpu
@pytest.mark.parametrize("icld,irng", [(2, 0), (5, 0), (3, 1)])
def test_in_place_view_equals_the_plain_entry(hip, oracle, icld, irng):
    plain = _plain_device(hip, oracle, icld, irng)
    for wide in (True, False):
        got = _view_call(hip, oracle, REFERENCE, wide, icld, irng)
        got["submask"] = got["submask"].view(np.uint32)
        for k in ALL:
            assert np.array_equal(got[k], plain[k]), (k, wide)


@gpu
def test_no_cloud_writes_exact_zeros(hip, oracle):
    import torch
    x, w = _inputs(oracle, 2)
    for nsamp, names in ((1, ALL), (3, FLOATS)):
        got = _plain_device(hip, oracle, 0, 0, names=names, nsamp=nsamp, step=140)
        for k in names:
            assert (got[k] == 0).all() and not np.signbit(got[k].astype(np.float64)).any(), k
        host = hip.mcica_cloud_cover(NCOL, NLAY, 0, SEED, 0, w["play"], w["cldfr"], nsamp=nsamp, outputs=names)
        for k in names:
            assert (host[k] == 0).all(), k
    # nothing is read: no input array is needed
    out = {"cldtot": torch.full((NCOL,), 9.0, dtype=torch.float64, device="cuda:0")}
    s = _stream()
    hip.mcica_cloud_cover_device({"ncol": NCOL, "nlay": NLAY}, out, 0, SEED, stream=s)
    hip.check(s)
    assert bool((out["cldtot"] == 0).all())
    # ... and in a float32 top-first C-order form inside nothing wider
    form = R4LFTOP
    fields, views = _output_fields(FLOATS, NCOL, NLAY, form, NCOL, 0)
    hip.mcica_cloud_cover_device({"ncol": NCOL, "nlay": NLAY}, views, 0, SEED, stream=s, form=form)
    hip.check(s)
    for k in FLOATS:
        assert bool((views[k] == 0).all()), k


BAD = [
    (dict(nsamp=0), "nsamp = 0"),
    (dict(nsamp=65), "RRTMG_LW_HIP_MAX_SAMPLES"),
    (dict(seedstep=0), "seedstep = 0"),
    (dict(seed=2147483647, nsamp=2, seedstep=1), "is not an int"),
    (dict(irng=1, nsamp=2), "irng = 1 with nsamp = 2"),
    (dict(names=()), "cldtot, cldcum, cldlay and submask"),
    (dict(drop="play"), "play"),
    (dict(drop="cldfr"), "cldfr"),
    (dict(icld=4, drop="alpha"), "alpha"),
    (dict(icld=5, drop="alpha"), "alpha"),
    (dict(nsamp=2, names=ALL), "submask"),
    (dict(icld=6), "ICLD"),
    (dict(icld=-1), "ICLD"),
]


@gpu
@pytest.mark.parametrize("kw,text", BAD, ids=["-".join(f"{k}_{len(v) if isinstance(v, tuple) else v}" for k, v in kw.items()) for kw, _ in BAD])
def test_refused_before_anything_is_written(hip, oracle, kw, text):
    import torch
    kw = dict(kw)
    icld, irng, seed = kw.get("icld", 2), kw.get("irng", 0), kw.get("seed", SEED)
    nsamp, step, names, drop = kw.get("nsamp", 1), kw.get("seedstep", 140), kw.get("names", FLOATS), kw.get("drop")
    x, w = _inputs(oracle, 4)                   # (with alpha)
    rc_want = 1 if "ICLD" in text else EARG     # (the reference's own stop: a physics error, as in the generator entry)
    # device entry, plain and view: the outputs keep their fill
    xd = _dev({k: v for k, v in x.items() if k not in ("dz", drop)})
    for view in (False, True):
        out = {k: torch.full((NLAY, NCOL) if k != "cldtot" else (NCOL,), -5.0, dtype=torch.float64, device="cuda:0") for k in names if k != "submask"}
        out = {k: (v.permute(1, 0) if v.dim() == 2 else v) for k, v in out.items()}
        if "submask" in names:
            out["submask"] = _mask_tensor(hip.mask_words())
        with pytest.raises(hip.RrtmgLwError, match=f"error {rc_want}: ") as e:
            hip.mcica_cloud_cover_device(xd, out, icld, seed, irng=irng, alpha=xd.get("alpha"), nsamp=nsamp, seedstep=step, stream=_stream(),
                                         ld=NCOL if view else None)
        assert text in str(e.value)
        torch.cuda.synchronize()
        for k, v in out.items():
            assert bool((v == (MASK_FILL if k == "submask" else -5.0)).all()), k
    # host entry
    ho = {k: np.full((NCOL, NLAY) if k != "cldtot" else (NCOL,), -5.0, order="F") for k in names if k != "submask"}
    if "submask" in names:
        ho["submask"] = np.full((NCOL, NLAY, hip.mask_words()), MASK_FILL, dtype=np.int32, order="F")
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp) if a is not None else C.cast(None, dp)
    irng_c = C.c_int(irng)
    rc = hip.lib().rrtmg_lw_hip_mcica_cloud_cover(C.c_int(NCOL), C.c_int(NLAY), C.c_int(icld), C.c_int(seed), C.c_int(nsamp), C.c_int(step),
                                                 C.byref(irng_c), *[ptr(None if k == drop else w[k]) for k in ("play", "cldfr", "alpha")],
                                                 *[ptr(ho.get(k)) for k in ALL])
    assert rc == rc_want and text in hip.lib().rrtmg_lw_hip_last_error().decode()
    for k, v in ho.items():
        assert (v == (MASK_FILL if k == "submask" else -5.0)).all(), k


@gpu
def test_null_irng_and_bad_dimensions_are_refused(hip, oracle):
    x, w = _inputs(oracle, 2)
    tot = np.full(NCOL, -5.0)
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp) if a is not None else C.cast(None, dp)
    fn = hip.lib().rrtmg_lw_hip_mcica_cloud_cover
    call = lambda ncol, nlay, irng: fn(C.c_int(ncol), C.c_int(nlay), C.c_int(2), C.c_int(SEED), C.c_int(1), C.c_int(140), irng,
                                       ptr(w["play"]), ptr(w["cldfr"]), ptr(None), ptr(tot), ptr(None), ptr(None), ptr(None))
    assert call(NCOL, NLAY, C.cast(None, C.POINTER(C.c_int))) == EARG and "irng" in hip.lib().rrtmg_lw_hip_last_error().decode()
    assert call(0, NLAY, C.byref(C.c_int(0))) == EARG
    assert call(NCOL, 604, C.byref(C.c_int(0))) == EARG
    assert call(NCOL, 3, C.byref(C.c_int(0))) == EARG and "four layers" in hip.lib().rrtmg_lw_hip_last_error().decode()
    assert (tot == -5.0).all()


@gpu
def test_column_batches_do_not_enter(hip, oracle):
    """the generator stage runs for all columns of the call at once: the smallest batch size, which makes three batches (64, 64, 3) of
    a solver call, changes nothing"""
    want = _want(oracle, 2, 0)
    hip.set_batch(64)
    try:
        _assert_equal(_plain_device(hip, oracle, 2, 0), want, ALL)
        _view_call(hip, oracle, R4, True, 2, 0)
    finally:
        hip.set_batch(0)


@gpu
def test_jump_tables_are_shared_with_the_fused_entries(hip, oracle):
    """a seed seen once rebuilds nothing, whichever entry saw it"""
    _plain_device(hip, oracle, 2, 0, names=FLOATS, nsamp=3, step=140)
    built = hip.kiss_tables_built()
    _plain_device(hip, oracle, 2, 0, names=FLOATS, nsamp=3, step=140)
    _plain_device(hip, oracle, 2, 0)
    assert hip.kiss_tables_built() == built


@gpu
def test_g256_library_counts_256_subcolumns(hip256, oracle):
    assert hip256.gpoints() == 256 and hip256.mask_words() == 8
    x, w = _inputs(oracle, 2)
    want = _want(oracle, 2, 0, gpoints=256)
    got = hip256.mcica_cloud_cover(NCOL, NLAY, 2, SEED, 0, w["play"], w["cldfr"], outputs=ALL)
    _assert_equal(got, want, ALL)
    assert got["submask"].shape == (NCOL, NLAY, 8) and ((got["cldtot"] > 0) & (got["cldtot"] < 1)).any()
    three = ccr.cover([_cldfmcl(oracle, 2, 0, SEED + s * 256, gpoints=256) for s in range(3)])
    _assert_equal(hip256.mcica_cloud_cover(NCOL, NLAY, 2, SEED, 0, w["play"], w["cldfr"], nsamp=3), three, FLOATS)


def test_python_entry_refuses_unknown_outputs():
    from rrtmg_lw_amd import api
    with pytest.raises(ValueError, match="unknown output"):
        api.mcica_cloud_cover(4, 4, 2, 0, 0, np.zeros((4, 4)), np.zeros((4, 4)), outputs=("cldtot", "cldmax"))
    with pytest.raises(ValueError, match="unknown output"):
        api.mcica_cloud_cover_device({"ncol": 4, "nlay": 4}, {"cldmax": None}, 2, 0)
