"""Time of the surface-temperature adjustment (rrtmg_lw_hip_adjust_tsfc_device / _device_as, kernels k_adjust_cf / k_adjust_lf) against
the library's calibration copy (rrtmg_lw_hip_calibrate_stream, k_calibrate) on the same number of bytes read plus written.

One process, HIP events around each kernel (the library's per-kernel event timing, rrtmg_lw_hip_profile_begin / _end), the runs
interleaved round by round: copy, form {8,0,0}, form {4,1,1}, copy of the float32 byte count, ...  Both flux sets.  Prints one JSON
line per measured item: median, minimum, maximum and quartiles of the rounds in milliseconds, the bytes moved, the rate they give and
the ratio to the copy's median.  The results of every form are compared with the numpy restatement on a slice of the columns first.
usage: python tools/adjust_tsfc_timing.py [--ncol 1000000] [--nlay 72] [--rounds 21] [--warmup 3]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

INS = ("plev", "dtsfc", "uflx", "dflx", "duflx_dt", "uflxc", "dflxc", "duflxc_dt")
OUTS = ("uflx_adj", "hr_adj", "uflxc_adj", "hrc_adj")


def traffic_bytes(ncol, nlay, real_bytes):
    """bytes the adjustment has to read plus write, both flux sets: seven level arrays and dtsfc in, two level and two layer arrays out"""
    return ncol * real_bytes * (7 * (nlay + 1) + 1 + 2 * (nlay + 1) + 2 * nlay)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    from rrtmg_lw_amd import api, arrays
    from rrtmg_lw_amd.arrays import ArrayForm

    if not torch.cuda.is_available():
        sys.exit("adjust_tsfc_timing: no GPU - a time is measured on the device or not at all")
    ncol, nlay = args.ncol, args.nlay
    api.rrtmg_lw_ini(1004.0, kdata=api.STANDIN_KDATA, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    heatfac = 9.8066 * 8.6400e4 / (1004.0 * 1.e2)

    # reference-form float64 inputs, generated on the device (column fastest: tensors of shape (rows, ncol))
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rnd = lambda rows, lo, hi: torch.rand((rows, ncol), generator=g, dtype=torch.float64, device="cuda:0") * (hi - lo) + lo
    ref = dict(plev=1013.0 - torch.cumsum(rnd(nlay + 1, 0.2, 1.0) * (1000.0 / (nlay + 1)), dim=0), dtsfc=rnd(1, -5.0, 5.0)[0].contiguous())
    for k, (lo, hi) in dict(uflx=(100, 500), uflxc=(100, 500), dflx=(0, 400), dflxc=(0, 400), duflx_dt=(0, 5), duflxc_dt=(0, 5)).items():
        ref[k] = rnd(nlay + 1, lo, hi)

    def in_form(form):
        """the inputs in `form` on the device: (rows, ncol) -> flipped / transposed / narrowed copies"""
        x = {}
        for k in INS:
            t = ref[k]
            if t.dim() == 2:
                if form.top_first:
                    t = t.flip(0)
                if form.layer_fastest:
                    t = t.t()
            x[k] = t.to(torch.float64 if form.real_bytes == 8 else torch.float32).contiguous()
        return x

    def check(form, x, out, cols=4096):
        """the first `cols` columns against the numpy restatement on the widened inputs"""
        n = min(cols, ncol)

        def host(t):           # -> (n, rows), surface first; t is (ncol, rows) in any storage order, or (rows, ncol)
            if t.dim() == 1:
                return t[:n].cpu().numpy()
            a = (t[:n] if t.shape[0] == ncol else t[:, :n].t()).cpu().numpy()
            return (a[:, ::-1] if form.top_first else a)
        w = {k: host(x[k]).astype(np.float64) for k in INS}
        dt = np.float64 if form.real_bytes == 8 else np.float32
        for u, d, du, ua, hr in (("uflx", "dflx", "duflx_dt", "uflx_adj", "hr_adj"), ("uflxc", "dflxc", "duflxc_dt", "uflxc_adj", "hrc_adj")):
            up = w[u] + w[du] * w["dtsfc"][:, None]
            net = up - w[d]
            h = heatfac * (net[:, :-1] - net[:, 1:]) / (w["plev"][:, :-1] - w["plev"][:, 1:])
            if not (np.array_equal(host(out[ua]), up.astype(dt)) and np.array_equal(host(out[hr]), h.astype(dt))):
                sys.exit(f"adjust_tsfc_timing: form {tuple(form)}: {ua} / {hr} differ from the numpy values")

    forms = (ArrayForm(8, 0, 0), ArrayForm(4, 1, 1))
    calls, nbytes = {}, {}
    for form in forms:
        x = dict(in_form(form), ncol=ncol, nlay=nlay)
        out = arrays.empty_like_form(OUTS, ncol, nlay, form, device="cuda:0", fill=0.0)
        f = None if form.is_reference else form
        calls[form] = (lambda x=x, out=out, f=f: api.adjust_tsfc_device(x, out, stream=stream, form=f))
        calls[form]()
        api.check(stream)
        check(form, x, out)
        nbytes[form] = traffic_bytes(ncol, nlay, form.real_bytes)
    del ref

    lib = api.lib()
    lib.rrtmg_lw_hip_calibrate_stream.argtypes = [ctypes.c_longlong]

    def timed(fn, kernel):
        """event time in ms of the one launch of `kernel` that fn() enqueues"""
        buf = ctypes.create_string_buffer(1 << 12)
        lib.rrtmg_lw_hip_profile_begin()
        fn()
        lib.rrtmg_lw_hip_profile_end(buf, len(buf))
        rows = dict((ln.split()[0], ln.split()[1:]) for ln in buf.value.decode().splitlines() if ln.strip())
        n, ms = rows[kernel]
        assert int(n) == 1, rows
        return float(ms)

    def copy(total):
        rc = lib.rrtmg_lw_hip_calibrate_stream(total // 2)            # reads total / 2 bytes and writes as many
        if rc != 0:
            sys.exit("calibrate_stream failed: " + lib.rrtmg_lw_hip_last_error().decode())

    items = []
    for form in forms:
        tag = "%d%d%d" % tuple(form)
        items.append(("copy_" + tag, lambda t=nbytes[form]: copy(t), "k_calibrate", nbytes[form]))
        items.append(("adjust_" + tag, calls[form], "k_adjust_lf" if form.layer_fastest else "k_adjust_cf", nbytes[form]))
    times = {name: [] for name, *_ in items}
    for r in range(args.warmup + args.rounds):
        for name, fn, kernel, _ in items:
            ms = timed(fn, kernel)
            if r >= args.warmup:
                times[name].append(ms)
    api.check(stream)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name, _, kernel, total in items:
        t = np.array(times[name])
        q1, q3 = np.percentile(t, [25, 75])
        yard = med["copy_" + name.split("_")[1]]
        print(json.dumps(dict(item=name, kernel=kernel, ncol=ncol, nlay=nlay, rounds=args.rounds, bytes=int(total),
                              median_ms=round(med[name], 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                              q1_ms=round(float(q1), 4), q3_ms=round(float(q3), 4), tb_per_s=round(total / med[name] / 1e9, 3),
                              ratio_to_copy=round(med[name] / yard, 3))))
    api.finalize()


if __name__ == "__main__":
    main()
