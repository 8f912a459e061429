"""What the solver entry costs (profiles/solver_entry.md): api.solve_device on device-resident cloudy columns whose inputs come from the
device optics entries (gas optics -> cloud optics -> cloud cover -> tau, odcld), for cloud = 0, 1, 2 and idrv = 0, 1.  Per case: the
bytes the entry must move - every input it reads once, every output once - over the median time, beside rrtmg_lw_hip_calibrate_stream
(one kernel that reads B bytes and writes B bytes with 16 B per lane) on the same byte count in the same run; the per-kernel HIP-event
times; and, as context only, the full rrtmg_lw_device call on the same columns (it reads a hundred times fewer bytes).
--big N: one N-column run (default 262 144: element offsets pass 2^31) whose last 64 columns must equal a 64-column call on them bit
for bit; the inputs are the measured columns repeated.

Wall time: samples of `--steps` calls between two device synchronisations, after warm-up calls.  Prints a markdown table and one JSON line.

    python tools/bench_solve.py [--ncol 65536] [--nlay 72] [--samples 7] [--steps 3] [--big 262144]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OUT = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc", "duflx_dt", "duflxc_dt")
# band -> cloud band (0-based) for ncbands = 1, 5, 16 (rtrn :343-349)
ICB = ([0] * 16, [0, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4], list(range(16)))


def kernel_ms(api, fn, steps):
    """per-kernel HIP-event ms per call of `fn`, over `steps` calls"""
    import torch
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    api.lib().rrtmg_lw_hip_profile_begin()
    for _ in range(steps):
        fn()
    api.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        k, n, ms = line.rsplit(" ", 2)
        out[k.strip()] = float(ms) / steps
    return out


def colfast(t):
    """the same values stored column-fastest (the reference form), logical shape kept"""
    r = list(reversed(range(t.dim())))
    return t.permute(*r).contiguous().permute(*r)


def optics_chain(api, d, stream, seed=1):
    """the solve entry's inputs for cloud = 1 and cloud = 2 from the device optics entries"""
    import torch
    from rrtmg_lw_amd import arrays
    from rrtmg_lw_amd.kspec import NGC
    ncol, nlay, ng, dev = d["ncol"], d["nlay"], api.gpoints(), d["plev"].device
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    g = dict(taug=f64(ng, nlay, ncol), fracs=f64(ng, nlay, ncol), planklay=f64(16, nlay, ncol), planklev=f64(16, nlay + 1, ncol),
             plankbnd=f64(16, ncol), dplankbnd_dt=f64(16, ncol))
    api.gas_optics_device(d, g, stream=stream, idrv=1)
    band = torch.repeat_interleave(torch.arange(16, device=dev), torch.as_tensor(list(NGC) if ng == 140 else [16] * 16, device=dev))
    x = dict(ncol=ncol, nlay=nlay, plev=d["plev"], emis=d["emis"], cldfr=d["cldfr"])
    x.update({k: v.permute(*reversed(range(v.dim()))) for k, v in g.items() if k != "taug"})
    co = {}
    for imca in (0, 1):
        o = arrays.empty_like_form(["taucloud", "secdiff"], ncol, nlay, arrays.REFERENCE, device=dev)
        o["ncbands"] = torch.zeros(ncol, dtype=torch.int32, device=dev)
        api.cloud_optics_device(d, o, imca=imca, stream=stream)
        co[imca] = o
    sec = co[0]["secdiff"]
    x["tau"] = colfast(sec[:, band][:, None, :] * (g["taug"].permute(2, 1, 0) + d["tauaer"][:, :, band]))
    del g["taug"]
    row = torch.searchsorted(torch.tensor([1, 5, 16], dtype=torch.int32, device=dev), co[0]["ncbands"])
    x["odcld1"] = colfast(torch.gather(sec, 1, torch.as_tensor(ICB, device=dev)[row])[:, None, :] * co[0]["taucloud"])
    x["odcld2"] = colfast(sec[:, None, :] * co[1]["taucloud"])
    m = torch.zeros(api.mask_words(), nlay, ncol, dtype=torch.int32, device=dev).permute(2, 1, 0)
    api.mcica_cloud_cover_device(dict(ncol=ncol, nlay=nlay, play=d["play"], cldfr=d["cldfr"]), {"submask": m}, 2, seed, irng=0, stream=stream)
    x["submask"] = m
    api.check(stream)
    return x


def outputs(ncol, nlay, dev):
    import torch
    return {k: torch.empty((nlay if k.startswith("hr") else nlay + 1, ncol), dtype=torch.float64, device=dev).t() for k in OUT}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=65536)
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--big", type=int, default=262144)
    args = ap.parse_args()

    import torch
    from rrtmg_lw_amd import api
    from rrtmg_lw_amd.synth import make_gcm_inputs
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = "cuda:0"
    api.rrtmg_lw_ini(1004.0, kdata=api.STANDIN_KDATA, device=0)
    ncol, nlay, ng, mw = args.ncol, args.nlay, api.gpoints(), api.mask_words()
    d = make_gcm_inputs(ncol, nlay, "cloudy", backend="torch", device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    x = optics_chain(api, d, stream)
    out = outputs(ncol, nlay, dev)
    med = statistics.median
    cells = ncol * nlay
    rows, results = [], []

    def time_it(fn):
        for _ in range(2):
            fn()
        api.check(stream)
        t = []
        for _ in range(args.samples):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) / args.steps * 1e3)
        return t

    for cloud in (0, 1, 2):
        xin = dict(x, odcld=x["odcld%d" % max(cloud, 1)])
        for idrv in (0, 1):
            read = 8 * (2 * ng * cells + 16 * cells + 17 * ncol * (nlay + 1) + (3 if idrv else 2) * 16 * ncol)
            read += (8 * cells if cloud == 1 else 0) + (8 * 16 * cells if cloud else 0) + (4 * mw * cells if cloud == 2 else 0)
            write = 8 * ((6 if idrv else 4) * ncol * (nlay + 1) + 2 * cells)
            half = (read + write) // 2 // 16 * 16

            def solve():
                api.solve_device(xin, out, cloud=cloud, idrv=idrv, stream=stream)

            def calibrate():
                api._check(api.lib().rrtmg_lw_hip_calibrate_stream(ctypes.c_longlong(half)))

            t = time_it(solve)
            kern = [kernel_ms(api, solve, args.steps) for _ in range(3)]
            cal = [kernel_ms(api, calibrate, 1)["k_calibrate"] for _ in range(3)]
            ks = {k: med([s[k] for s in kern]) for k in sorted(kern[0])}
            rate, crate = (read + write) / med(t) / 1e6, 2 * half / med(cal) / 1e6
            rows.append(f"| {cloud} | {idrv} | {(read + write) / 1e9:.2f} | {med(t):.2f} | {min(t):.2f} | {max(t):.2f} | {rate:.0f} | {med(cal):.2f} | {crate:.0f} | {rate / crate:.2f} | "
                        + ", ".join(f"{k} {v:.2f}" for k, v in ks.items()) + " |")
            results.append({"cloud": cloud, "idrv": idrv, "bytes": read + write, "wall_ms": {"median": med(t), "min": min(t), "max": max(t)},
                            "kernels_ms": ks, "calibrate_ms": med(cal), "fraction_of_stream_rate": rate / crate})
    full = {}
    ref = outputs(ncol, nlay, dev)
    for icld in (0, 1):
        full[icld] = med(time_it(lambda: api.rrtmg_lw_device(d, ref, icld=icld, idrv=0, stream=stream)))
    print(f"{ncol} columns x {nlay} layers, {ng} g-points; {100 * float((d['cldfr'] >= 1e-6).double().mean()):.1f} % of the layers cloudy; "
          f"{args.samples} samples of {args.steps} calls; workspace {api.workspace_bytes() / 1e9:.2f} GB")
    print("| cloud | idrv | GB to move | median ms | min | max | GB/s | k_calibrate ms | its GB/s | fraction | kernels (HIP events, ms) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    print(f"context: rrtmg_lw_device on the same columns, idrv = 0: icld 0 {full[0]:.2f} ms, icld 1 {full[1]:.2f} ms")
    big = None
    if args.big:
        reps = (args.big + ncol - 1) // ncol
        tile = lambda t: colfast(torch.cat([t] * reps, dim=0)[:args.big])
        xb = {k: tile(v) for k, v in x.items() if torch.is_tensor(v) and k not in ("odcld1", "odcld2")}
        xb.update(ncol=args.big, nlay=nlay, odcld=tile(x["odcld2"]))
        del x, xin
        ob = outputs(args.big, nlay, dev)
        api.solve_device(xb, ob, cloud=2, idrv=1, stream=stream)
        api.check(stream)
        xs = {k: colfast(v[args.big - 64:]) for k, v in xb.items() if torch.is_tensor(v)}
        xs.update(ncol=64, nlay=nlay)
        os_ = outputs(64, nlay, dev)
        api.solve_device(xs, os_, cloud=2, idrv=1, stream=stream)
        api.check(stream)
        same = all(bool(torch.equal(ob[k][args.big - 64:], os_[k])) for k in OUT)
        finite = all(bool(torch.isfinite(ob[k]).all()) for k in OUT)
        big = {"ncol": args.big, "elements": args.big * nlay * ng, "last_64_bitwise_equal": same, "finite": finite}
        print(f"{args.big} columns, cloud 2, idrv 1: {args.big * nlay * ng} elements per array (2^31 = {2 ** 31}); the last 64 columns "
              f"{'equal' if same else 'DIFFER FROM'} a 64-column call on them bit for bit; all outputs finite: {finite}")
    print(json.dumps({"ncol": ncol, "nlay": nlay, "cases": results, "rrtmg_lw_device_ms": full, "big": big}))
    api.finalize()
    if big and not (big["last_64_bitwise_equal"] and big["finite"]):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
