"""What the in-place view entry costs (profiles/device_views.md).  Three ways to solve the same columns of fields `--ld` columns wide, on
one GPU, interleaved in one process:

    (a) plain    rrtmg_lw_device on contiguous arrays that hold the call's columns and nothing else
    (b) view     rrtmg_lw_device(..., ld=ld): the view entry {8,0,0,ld} on the call's columns where they lie in the fields
    (c) gather   what a host did before the view entries: torch copies the columns out of the fields into the contiguous arrays, the
                 plain entry runs, torch copies the outputs back into the fields

Each sample is the wall time of `--steps` calls between two device synchronisations; the samples of the three variants alternate
(a, b, c, a, b, c, ...), so that whatever else the machine does meets all three alike.  Before anything is timed the outputs of (b) and (c)
are compared with those of (a), bit for bit.  Prints a markdown table: median, minimum and maximum of the samples in ms per call, the
spread (maximum - minimum) and the rate.

    python tools/device_view_timing.py [--ncol 1000000 16384] [--nlay 72] [--ld 1048576] [--samples 7]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(ncol, nlay, ld, config, dev):
    """the inputs of `ncol` columns twice: contiguous, and as the first columns of fields ld wide that hold NaN elsewhere"""
    import torch
    from rrtmg_lw_amd import arrays
    from rrtmg_lw_amd.api import _CLD_ORDER, _GCM_ORDER
    from rrtmg_lw_amd.synth import make_gcm_inputs
    names = _GCM_ORDER + _CLD_ORDER
    ref = arrays.REFERENCE
    cont = arrays.empty_like_form(names, ncol, nlay, ref, device=dev)
    fields = arrays.empty_like_form(names, ld, nlay, ref, device=dev, fill=float("nan"))
    slab, scal = 131072, {}
    for s in range(0, ncol, slab):
        n = min(slab, ncol - s)
        p = make_gcm_inputs(n, nlay, config, col0=s, backend="torch", device=dev)
        for k in names:
            arrays.field_view(cont[k], k, ref, n, s).copy_(p[k])
            arrays.field_view(fields[k], k, ref, n, s).copy_(p[k])
        scal = {k: v for k, v in p.items() if not torch.is_tensor(v)}
    scal["ncol"] = ncol
    views = {k: arrays.field_view(fields[k], k, ref, ncol, 0) for k in names}
    return dict(scal, **cont), dict(scal, **views), fields


def measure(ncol, nlay, ld, config, steps, samples, dev, per_kernel=False):
    import torch
    from rrtmg_lw_amd import api, arrays
    ref = arrays.REFERENCE
    d_cont, d_view, fields = build(ncol, nlay, ld, config, dev)
    outs = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc") + (("duflx_dt", "duflxc_dt") if d_cont["idrv"] == 1 else ())
    o_cont = arrays.empty_like_form(outs, ncol, nlay, ref, device=dev)
    o_field = arrays.empty_like_form(outs, ld, nlay, ref, device=dev, fill=float("nan"))
    o_view = {k: arrays.field_view(o_field[k], k, ref, ncol, 0) for k in outs}
    stream = torch.cuda.current_stream().cuda_stream
    ins = [k for k, v in d_cont.items() if torch.is_tensor(v)]

    def plain():
        api.rrtmg_lw_device(d_cont, o_cont, stream=stream)

    def view():
        api.rrtmg_lw_device(d_view, o_view, stream=stream, ld=ld)

    def gather():
        for k in ins:
            d_cont[k].copy_(d_view[k])
        api.rrtmg_lw_device(d_cont, o_cont, stream=stream)
        for k in outs:
            o_view[k].copy_(o_cont[k])

    variants = (("(a) plain, contiguous", plain), ("(b) view {8,0,0,%d}" % ld, view), ("(c) gather, plain, scatter", gather))
    # same results first
    plain()
    api.check(stream)
    want = {k: o_cont[k].clone() for k in outs}
    for name, fn in variants[1:]:
        for k in outs:
            o_field[k].fill_(float("nan"))
        fn()
        api.check(stream)
        for k in outs:
            assert torch.equal(o_view[k], want[k]), (name, k)
    for _, fn in variants:                       # warm-up: every variant, every lazily made stream, workspace and graph
        for _ in range(3):
            fn()
    api.check(stream)
    times = {name: [] for name, _ in variants}
    for _ in range(samples):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    api.check(stream)
    kernels = None
    if per_kernel:
        # the library's own per-kernel HIP-event times (rrtmg_lw_hip_profile_begin / _end), (a) and (b) in passes of their own
        import ctypes
        kernels = {}
        for name, fn in variants[:2]:
            buf = ctypes.create_string_buffer(1 << 16)
            torch.cuda.synchronize()
            api.lib().rrtmg_lw_hip_profile_begin()
            for _ in range(steps):
                fn()
            api.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
            for line in buf.value.decode().splitlines():
                k, n, ms = line.rsplit(" ", 2)
                kernels.setdefault(k, {})[name] = float(ms) / steps
    rows = []
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        rows.append((name, med, min(t), max(t), max(t) - min(t), ncol / med / 1e3))
    return rows, kernels, [name for name, _ in variants[:2]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, nargs="+", default=[1_000_000, 16384])
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--ld", type=int, default=1_048_576)
    ap.add_argument("--config", default="cloudy")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--kernels", action="store_true", help="also the per-kernel times of (a) and (b), summed over a call's launches")
    ap.add_argument("--steps", type=int, default=0, help="calls per sample (0: 5 for a call of 100 000 columns or more, 100 below)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("device_view_timing.py needs a GPU (the solver has no CPU path)")
    from rrtmg_lw_amd import api
    dev = torch.device("cuda", 0)
    api.rrtmg_lw_ini(1004.0, kdata=api.REAL_KDATA if os.path.exists(api.REAL_KDATA) else api.STANDIN_KDATA, device=0)
    for ncol in args.ncol:
        steps = args.steps or (5 if ncol >= 100_000 else 100)
        rows, kernels, ab = measure(ncol, args.nlay, args.ld, args.config, steps, args.samples, dev, args.kernels)
        print(f"\n{ncol} columns x {args.nlay} layers in fields {args.ld} wide, {args.config}, icld = 2 (rtrnmr); {args.samples} samples of {steps} calls each, interleaved\n")
        print("| variant | median ms | min ms | max ms | spread ms | M columns/s (median) |")
        print("|---|---|---|---|---|---|")
        for name, med, lo, hi, spread, rate in rows:
            print(f"| {name} | {med:.3f} | {lo:.3f} | {hi:.3f} | {spread:.3f} | {rate:.2f} |")
        if kernels:
            print("\n| kernel (ms per call, all its launches) | (a) | (b) | (b) - (a) |")
            print("|---|---|---|---|")
            for k, v in sorted(kernels.items(), key=lambda kv: -abs(kv[1].get(ab[1], 0.0) - kv[1].get(ab[0], 0.0))):
                a, b = v.get(ab[0], 0.0), v.get(ab[1], 0.0)
                print(f"| {k} | {a:.3f} | {b:.3f} | {b - a:+.3f} |")
        sys.stdout.flush()
        torch.cuda.empty_cache()
    api.finalize()


if __name__ == "__main__":
    main()
