#!/usr/bin/env python3
"""Cost of the gas-optics device entry (include/rrtmg_lw_hip.h, "Gas optics and Planck sources"): --ncol columns in device-resident calls
of --call columns each (the outputs take ~180 KB per 72-layer column: one call's set is reused), every call timed with HIP events on the
caller's stream.  One JSON line per config: ms per 1e6 columns (median round), bytes written per column, the achieved write rate, and for
comparison the rate of a plain device fill of the same bytes (torch fill_).
usage: python tools/optics_timing.py [--ncol N] [--call C] [--nlay L] [--configs clear,cloudy_orography] [--rounds R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1_048_576)
    ap.add_argument("--call", type=int, default=131072)
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--configs", default="clear")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--planck", type=int, default=1, help="1: all Planck outputs as well, 0: taug and fracs only")
    args = ap.parse_args()

    import torch
    from rrtmg_lw_amd import api
    from rrtmg_lw_amd.synth import make_gcm_inputs
    dev = torch.device("cuda", 0)
    api.rrtmg_lw_ini(1004.0, kdata=api.REAL_KDATA if os.path.exists(api.REAL_KDATA) else api.STANDIN_KDATA, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    ng, nlay, nc = api.gpoints(), args.nlay, args.call
    e = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    for cfg in args.configs.split(","):
        d = make_gcm_inputs(nc, nlay, cfg, col0=0, backend="torch", device=dev)
        out = dict(taug=e(ng, nlay, nc), fracs=e(ng, nlay, nc))
        if args.planck:
            out.update(planklay=e(16, nlay, nc), planklev=e(16, nlay + 1, nc), plankbnd=e(16, nc))
        per_col = sum(t.numel() for t in out.values()) * 8 // nc
        calls = max(1, args.ncol // nc)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        api.gas_optics_device(d, out, stream=stream, idrv=0)          # warm-up: workspace, first launch
        api.check(stream)
        rounds = []
        for _ in range(args.rounds):
            t = 0.0
            for _ in range(calls):
                ev[0].record()
                api.gas_optics_device(d, out, stream=stream, idrv=0)
                ev[1].record()
                ev[1].synchronize()
                t += ev[0].elapsed_time(ev[1])
            rounds.append(t)
        api.check(stream)
        ms = sorted(rounds)[len(rounds) // 2] * 1e6 / (calls * nc)
        # the same bytes written by a plain fill (the write rate this box reaches without any arithmetic)
        fill = []
        for _ in range(3):
            ev[0].record()
            for t_ in out.values():
                t_.fill_(1.0)
            ev[1].record()
            ev[1].synchronize()
            fill.append(ev[0].elapsed_time(ev[1]))
        fill_ms = min(fill)
        print(json.dumps(dict(config=cfg, nlay=nlay, gpoints=ng, columns=calls * nc, call_columns=nc, planck=bool(args.planck),
                              ms_per_1e6_columns=round(ms, 2), rounds_ms=[round(r, 2) for r in rounds], bytes_per_column=per_col,
                              write_TBps=round(per_col * 1e6 / (ms * 1e-3) / 1e12, 3),
                              fill_TBps=round(per_col * nc / (fill_ms * 1e-3) / 1e12, 3))), flush=True)
        del d, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
