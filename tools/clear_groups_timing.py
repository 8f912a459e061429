#!/usr/bin/env python3
"""Timing of the cloud-free sweep of cloudy calls (rrtmg_lw_hip_set_clear_groups; profiles/clear_groups.md), device-resident calls, the
settings taken in turn several times so that drift of the box cancels; every setting's outputs are compared bit for bit with the first's.
  --mode coherent   1e6 "cloudy" columns whose cloud is zeroed in whole windows of 256 consecutive columns, 30 % of the windows (clear
                    regions as a model has them): the switch off / on, column order off, and per-kernel HIP-event times of each
  --mode bonus      the benchmark's fields: column order off, on with bonus 0 (the criterion of the parent), on with the bonuses of --bonus
usage: python tools/clear_groups_timing.py --mode coherent|bonus [--configs ..] [--bonus 12,18,24] [--rounds 3]"""
import argparse, ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="coherent", choices=["coherent", "bonus"])
ap.add_argument("--configs", default="cloudy,cloudy_towers,cloudy_scatter,cloudy_deep,cloudy_orography")
ap.add_argument("--bonus", default="12,18,24", help="per cent of nlay (RRTMG_LW_COLSORT_CLEAR)")
ap.add_argument("--ncol", type=int, default=1000000)
ap.add_argument("--nlay", type=int, default=72)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--clear-share", type=float, default=0.30)
args = ap.parse_args()
import torch
from rrtmg_lw_amd import api
from rrtmg_lw_amd.synth import make_gcm_inputs
from rrtmg_lw_amd.shard import output_rows, output_views
dev = torch.device("cuda", 0)
api.rrtmg_lw_ini(1004.0, kdata=api.REAL_KDATA if os.path.exists(api.REAL_KDATA) else api.STANDIN_KDATA, device=0)
stream = torch.cuda.current_stream().cuda_stream


def field(cfg):
    """the benchmark's columns on the device, column-fastest (as bench.py builds them)"""
    slab = 131072
    parts = [make_gcm_inputs(min(slab, args.ncol - s), args.nlay, cfg, col0=s, backend="torch", device=dev) for s in range(0, args.ncol, slab)]
    d = dict(parts[0])
    d["ncol"] = args.ncol
    for k, v in parts[0].items():
        if torch.is_tensor(v) and len(parts) > 1:
            cat = torch.cat([p[k] for p in parts], dim=1 if k == "taucld" else 0)
            nd = cat.dim()
            d[k] = cat.permute(*reversed(range(nd))).contiguous().permute(*reversed(range(nd))) if nd > 1 else cat.contiguous()
    return d


def kernel_times(d, o):
    """HIP-event ms per call of every kernel family member (rrtmg_lw_hip_profile_begin / _end), one call"""
    buf = ctypes.create_string_buffer(1 << 16)
    api.lib().rrtmg_lw_hip_profile_begin()
    api.rrtmg_lw_device(d, o, stream=stream)
    api.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
    rows = [ln.split() for ln in buf.value.decode().splitlines() if ln.strip()]
    return {r[0]: (int(r[1]), float(r[2])) for r in rows}


def ab(d, settings):
    """ms per call of every setting (name, apply), taken in turn args.rounds times: "best (+ worst - best)"; the outputs compared with the
    first setting's"""
    idrv = d["idrv"]
    bufs = [torch.zeros((output_rows(args.nlay, idrv), args.ncol), dtype=torch.float64, device=dev) for _ in settings]
    times = [[] for _ in settings]
    for _ in range(args.rounds):
        for i, (_, apply) in enumerate(settings):
            apply()
            o = output_views(bufs[i], args.nlay, idrv)
            api.rrtmg_lw_device(d, o, stream=stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                api.rrtmg_lw_device(d, o, stream=stream)
            torch.cuda.synchronize()
            times[i].append(1e3 * (time.perf_counter() - t0) / args.reps)
    api.check(stream)
    same = all(bool(torch.equal(bufs[0].view(torch.int64), b.view(torch.int64))) for b in bufs[1:])
    return [f"{min(t):.2f} (+{max(t) - min(t):.2f})" for t in times], same, bufs


if args.mode == "coherent":
    d = field("cloudy")
    nwin = (args.ncol + 255) // 256
    g = torch.Generator().manual_seed(5)
    clear = (torch.rand(nwin, generator=g) < args.clear_share).repeat_interleave(256)[:args.ncol].to(dev)
    for k in ("cldfr", "cliqwp", "cicewp"):
        d[k][clear] = 0.0
    print(f"{args.ncol} cloudy columns, cloud zeroed in {100 * float(clear.float().mean()):.1f} % of them (whole windows of 256)")
    api.set_column_sort(0, -1)
    settings = [("switch off", lambda: api.set_clear_groups(0)), ("switch on", lambda: api.set_clear_groups(1))]
    best, same, bufs = ab(d, settings)
    print("| " + " | ".join(s[0] for s in settings) + " | bit-identical |\n|---|---|---|")
    print("| " + " | ".join(best) + f" | {same} |", flush=True)
    for i, (name, apply) in enumerate(settings):
        apply()
        kt = kernel_times(d, output_views(bufs[i], args.nlay, d["idrv"]))
        fam = {}
        for k, (n, ms) in kt.items():
            f = k.split("<")[0]
            fam[f] = fam.get(f, 0.0) + ms
        print(f"{name}: " + "  ".join(f"{k} {v:.2f}" for k, v in sorted(fam.items()) if v >= 0.05))
        print("   " + "  ".join(f"{k} {ms:.2f}" for k, (n, ms) in sorted(kt.items()) if k.startswith("k_sweep")), flush=True)
else:
    bonuses = [int(b) for b in args.bonus.split(",")]
    settings = [("off", lambda: api.set_column_sort(0, -1)), ("on, bonus 0", lambda: (api.set_column_sort(1, -1), api.set_column_sort_clear(0)))]
    settings += [(f"on, bonus {b}", (lambda b=b: (api.set_column_sort(1, -1), api.set_column_sort_clear(b)))) for b in bonuses]
    print(f"threshold {api.column_sort_min()} block-levels, ms per call of {args.ncol} columns: best (+ spread) of {args.rounds} rounds of {args.reps} calls")
    print("| config | " + " | ".join(s[0] for s in settings) + " | bit-identical |")
    print("|---|" + "---|" * (len(settings) + 1))
    for cfg in args.configs.split(","):
        d = field(cfg)
        best, same, bufs = ab(d, settings)
        print(f"| {cfg} | " + " | ".join(best) + f" | {same} |", flush=True)
        del d, bufs
        torch.cuda.empty_cache()
api.finalize()
