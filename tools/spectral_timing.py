#!/usr/bin/env python3
"""Cost of the spectral outputs (include/rrtmg_lw_hip.h, "Spectral (per-band) fluxes") on the device-resident step: broadband only,
spectral total sky only (uflxs, dflxs) and spectral total + clear sky (all four), ALTERNATING in one process, each step timed with
HIP events on the caller's stream.  One JSON line per (config, variant): median / min ms per step, the ratio to the broadband median,
and the variant's roofline bytes - the step's measured traffic (--traffic_gb, per 1e6 columns at 72 layers: the PMC figure of DESIGN
section 8) plus the spectral arrays' stores, 16 (nlay + 1) x 8 B per column and array (9 344 B at 72 layers).
usage: python tools/spectral_timing.py [--ncol N] [--nlay L] [--configs cloudy,cloudy_scatter] [--rounds R] [--traffic_gb G]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1_000_000)
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--configs", default="cloudy,cloudy_scatter")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--traffic_gb", type=float, default=236.0, help="measured HBM bytes of a broadband step per 1e6 columns (GB)")
    args = ap.parse_args()

    import torch
    from rrtmg_lw_amd import api
    from rrtmg_lw_amd.synth import make_gcm_inputs
    from rrtmg_lw_amd.shard import output_rows, output_views
    dev = torch.device("cuda", 0)
    api.rrtmg_lw_ini(1004.0, kdata=api.REAL_KDATA if os.path.exists(api.REAL_KDATA) else api.STANDIN_KDATA, device=0)
    ncol, nlay = args.ncol, args.nlay
    stream = torch.cuda.current_stream().cuda_stream
    spec_bytes = 16 * (nlay + 1) * 8          # per column and array
    for cfg in args.configs.split(","):
        slab = 131072
        parts = [make_gcm_inputs(min(slab, ncol - s), nlay, cfg, col0=s, backend="torch", device=dev) for s in range(0, ncol, slab)]
        d = dict(parts[0])
        d["ncol"] = ncol
        for k, v in parts[0].items():
            if torch.is_tensor(v) and len(parts) > 1:
                cat = torch.cat([p[k] for p in parts], dim=1 if k == "taucld" else 0)
                nd = cat.dim()
                d[k] = cat.permute(*reversed(range(nd))).contiguous().permute(*reversed(range(nd))) if nd > 1 else cat.contiguous()
        del parts
        idrv = d["idrv"]
        buf = torch.zeros((output_rows(nlay, idrv), ncol), dtype=torch.float64, device=dev)
        base = output_views(buf, nlay, idrv)
        spec = {k: torch.zeros((16, nlay + 1, ncol), dtype=torch.float64, device=dev) for k in ("uflxs", "dflxs", "uflxcs", "dflxcs")}
        variants = {
            "broadband": dict(base),
            "spectral_total": dict(base, uflxs=spec["uflxs"], dflxs=spec["dflxs"]),
            "spectral_total_clear": dict(base, **spec),
        }
        times = {v: [] for v in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for r in range(args.warmup + args.rounds):
            for name, o in variants.items():          # alternating: drifts of clock or temperature hit every variant alike
                ev[0].record()
                api.rrtmg_lw_device(d, o, stream=stream)
                ev[1].record()
                ev[1].synchronize()
                if r >= args.warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]))
        api.check(stream)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for name, ts in times.items():
            narr = {"broadband": 0, "spectral_total": 2, "spectral_total_clear": 4}[name]
            traffic = args.traffic_gb * 1e9 * ncol / 1e6 * (nlay / 72.0) + narr * spec_bytes * ncol
            print(json.dumps(dict(config=cfg, variant=name, columns=ncol, nlay=nlay, steps=len(ts), median_ms=round(med[name], 3),
                                  min_ms=round(min(ts), 3), ratio_to_broadband=round(med[name] / med["broadband"], 4),
                                  spectral_bytes=narr * spec_bytes * ncol, roofline_bytes=round(traffic),
                                  roofline_TBps=round(traffic / (med[name] * 1e-3) / 1e12, 3))))
        del d, buf, base, spec, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
