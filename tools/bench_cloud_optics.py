"""What the cloud-optics device entry costs (profiles/cloud_optics.md): api.cloud_optics_device with all three outputs on device-resident
columns, beside rrtmg_lw_hip_calibrate_stream - one kernel that reads B bytes and writes B bytes with 16 B per lane - for the same
traffic: 2 B = the bytes the entry has to move (every input read once, every output written once).

Wall time: samples of `--steps` calls between two device synchronisations, after warm-up calls.  Kernel times: the library's per-kernel
HIP-event times (rrtmg_lw_hip_profile_begin / _end) in passes of their own, the entry's and the calibration kernel's alternating.
Prints a markdown table and one JSON line.

    python tools/bench_cloud_optics.py [--ncol 131072] [--nlay 72] [--imca 0] [--samples 7] [--steps 5]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=131072)
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--imca", type=int, default=0)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()

    import torch
    from rrtmg_lw_amd import api, arrays
    from rrtmg_lw_amd.synth import make_gcm_inputs
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = "cuda:0"
    api.rrtmg_lw_ini(1004.0, kdata=api.STANDIN_KDATA, device=0)
    ncol, nlay = args.ncol, args.nlay
    d = make_gcm_inputs(ncol, nlay, "cloudy", backend="torch", device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = arrays.empty_like_form(("taucloud", "secdiff"), ncol, nlay, arrays.REFERENCE, device=dev)
    out["ncbands"] = torch.empty((ncol,), dtype=torch.int32, device=dev)
    cells = ncol * nlay
    read = 8 * (5 * cells + 16 * cells + cells + ncol * (nlay + 1))         # five layer arrays, taucld, h2ovmr, plev
    write = 8 * (16 * cells + 16 * ncol) + 4 * ncol
    half = (read + write) // 2 // 16 * 16

    def optics():
        api.cloud_optics_device(d, out, imca=args.imca, stream=stream)

    def calibrate():
        api._check(api.lib().rrtmg_lw_hip_calibrate_stream(ctypes.c_longlong(half)))

    for _ in range(3):
        optics()
    api.check(stream)
    cloudy = float((out["taucloud"] != 0).any(dim=2).double().mean())
    times = []
    for _ in range(args.samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            optics()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / args.steps * 1e3)
    api.check(stream)
    kern, cal = [], []
    for _ in range(args.samples):
        kern.append(kernel_ms(api, optics, args.steps))
        cal.append(kernel_ms(api, calibrate, 1)["k_calibrate"])
    api.check(stream)
    med = lambda v: statistics.median(v)
    names = sorted(kern[0])
    ks = {k: med([s[k] for s in kern]) for k in names}
    print(f"{ncol} columns x {nlay} layers, imca = {args.imca}, inflglw / iceflglw / liqflglw = {d['inflglw']} / {d['iceflglw']} / {d['liqflglw']}; "
          f"{100 * cloudy:.1f} % of the cells hold a cloud optical depth; {args.samples} samples of {args.steps} calls")
    print(f"bytes: {read / 1e6:.1f} MB read + {write / 1e6:.1f} MB written = {(read + write) / 1e6:.1f} MB")
    print("| what | median ms | min | max | GB/s at the median |")
    print("|---|---|---|---|---|")
    print(f"| cloud_optics_device, wall per call | {med(times):.3f} | {min(times):.3f} | {max(times):.3f} | {(read + write) / med(times) / 1e6:.0f} |")
    for k in names:
        v = [s[k] for s in kern]
        print(f"| {k} (HIP events) | {med(v):.3f} | {min(v):.3f} | {max(v):.3f} | |")
    tot = sum(ks.values())
    print(f"| both kernels | {tot:.3f} | | | {(read + write) / tot / 1e6:.0f} |")
    print(f"| k_calibrate, {2 * half / 1e6:.1f} MB (HIP events) | {med(cal):.3f} | {min(cal):.3f} | {max(cal):.3f} | {2 * half / med(cal) / 1e6:.0f} |")
    print(json.dumps({"ncol": ncol, "nlay": nlay, "imca": args.imca, "bytes": read + write, "wall_ms": {"median": med(times), "min": min(times), "max": max(times)},
                      "kernels_ms": ks, "calibrate_ms": med(cal)}))
    api.finalize()


if __name__ == "__main__":
    main()
