"""What the cloud-cover entry costs (profiles/mcica_cloud_cover.md).  Two ways to get cldtot, cldcum and cldlay of the same device-resident
columns on one GPU, interleaved in one process:

    (a) cover    api.mcica_cloud_cover_device: the generator stage and k_cloudcover, which counts the packed mask
    (b) expand   what a host could do before: api.mcica_subcol_device materialises the four (NG, ncol, nlay) float64 arrays, torch
                 reduces cldfmcl (sum over the sub-columns; running maximum from the top layer down, then the sum)

Each sample is the wall time of `--steps` calls between two device synchronisations; the samples of the two alternate (a, b, a, b, ...),
so that whatever else the machine does meets both alike.  Before anything is timed the three outputs of (b) are compared with those of
(a), bit for bit.  Then, in passes of their own, the library's per-kernel HIP-event times (rrtmg_lw_hip_profile_begin / _end) of (a) and
of the fused solver entry with the same arguments: k_subcol_kiss here and there, and k_cloudcover.  Prints a markdown table and one JSON
line.

    python tools/bench_cloud_cover.py [--ncol 131072] [--nlay 72] [--icld 2] [--samples 7] [--steps 3]"""
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
    ap.add_argument("--icld", type=int, default=2)
    ap.add_argument("--seed", type=int, default=280)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-solver", action="store_true", help="skip the fused solver pass (the generator's time inside it)")
    args = ap.parse_args()

    import torch
    from rrtmg_lw_amd import api, arrays
    from rrtmg_lw_amd.synth import make_gcm_inputs
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = "cuda:0"
    api.rrtmg_lw_ini(1004.0, kdata=api.STANDIN_KDATA, device=0)
    ncol, nlay, icld, seed = args.ncol, args.nlay, args.icld, args.seed
    ng = api.gpoints()
    d = make_gcm_inputs(ncol, nlay, "cloudy", backend="torch", device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    names = ("cldtot", "cldcum", "cldlay")
    out = arrays.empty_like_form(names, ncol, nlay, arrays.REFERENCE, device=dev)
    sub = {k: torch.empty((nlay, ncol, ng), dtype=torch.float64, device=dev) for k in ("cldfmcl", "ciwpmcl", "clwpmcl", "taucmcl")}
    sub.update({k: torch.empty((nlay, ncol), dtype=torch.float64, device=dev) for k in ("reicmcl", "relqmcl")})
    old = {}
    den = torch.full((), float(ng), dtype=torch.float64, device=dev)        # (a tensor: torch divides by it; a Python scalar it would invert and multiply by)

    def cover():
        api.mcica_cloud_cover_device(d, out, icld, seed, stream=stream)

    def expand():
        api.mcica_subcol_device(d, sub, icld, seed, 0, stream=stream)
        c = sub["cldfmcl"]                                                  # (nlay, ncol, NG), zeros and ones
        old["cldlay"] = c.sum(dim=2) / den
        seen = torch.cummax(c.flip(0), dim=0).values.flip(0)                # cloudy in this layer or any above it
        old["cldcum"] = seen.sum(dim=2) / den
        old["cldtot"] = old["cldcum"][0]

    # same results first
    cover()
    expand()
    api.check(stream)
    for k in names:
        a, b = out[k], old[k] if k == "cldtot" else old[k].t()
        assert torch.equal(a, b), k
    tot = out["cldtot"]
    partial = float(((tot > 0) & (tot < 1)).double().mean())
    for fn in (cover, expand):
        for _ in range(2):
            fn()
    api.check(stream)
    variants = (("(a) cover", cover), ("(b) expand + torch", expand))
    times = {name: [] for name, _ in variants}
    for _ in range(args.samples):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    api.check(stream)
    kern = {"cover": kernel_ms(api, cover, args.steps)}
    api.check(stream)
    if not args.no_solver:
        fl = arrays.empty_like_form(("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc"), ncol, nlay, arrays.REFERENCE, device=dev)
        solver = lambda: api.rrtmg_lw_mcica_subcol_device(d, fl, seed, 0, icld=icld, stream=stream)
        solver()
        api.check(stream)
        kern["fused"] = kernel_ms(api, solver, 1)
        api.check(stream)

    print(f"{ncol} columns x {nlay} layers, icld = {icld}, NG = {ng}; {100 * partial:.1f} % of the columns partly covered; "
          f"{args.samples} samples of {args.steps} calls, alternating")
    print("| variant | median ms | min | max | columns/s |")
    print("|---|---|---|---|---|")
    res = {}
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        res[name] = {"median_ms": med, "min_ms": min(t), "max_ms": max(t)}
        print(f"| {name} | {med:.3f} | {min(t):.3f} | {max(t):.3f} | {ncol / med * 1e3:.3e} |")
    print("kernel times (HIP events, ms per call):")
    for where, ks in kern.items():
        for k in sorted(ks):
            if where == "cover" or k.startswith("k_subcol"):
                print(f"  {where:6s} {k:24s} {ks[k]:.3f}")
    mask_bytes = 4 * ((ng + 31) // 32) * nlay * ncol
    kc = kern["cover"].get("k_cloudcover<f64>")
    if kc:
        print(f"  k_cloudcover reads {mask_bytes / 1e6:.1f} MB of mask and writes {8 * ncol * (2 * nlay + 1) / 1e6:.1f} MB: "
              f"{(mask_bytes + 8 * ncol * (2 * nlay + 1)) / kc / 1e6:.1f} GB/s")
    print(json.dumps({"ncol": ncol, "nlay": nlay, "icld": icld, "ng": ng, "times": res, "kernels": kern}))
    api.finalize()


if __name__ == "__main__":
    main()
