#!/usr/bin/env python3
"""End-to-end rate of the float32 host entries (rrtmg_lw_hip_run_nomcica_r4, rrtmg_lw_hip_run_mcica_subcol_r4) beside the float64 ones,
on the columns of tools/e2e_timing.py.  Three ways, the same columns, one process, interleaved round by round:
    f64      float64 arrays through the float64 entry;
    r4       float32 arrays through the float32 entry;
    widened  float32 arrays widened with numpy into float64 temporaries around the float64 entry, the outputs narrowed with numpy -
             what a host built with 4-byte reals has to do without the float32 entries.
Each way with its persistent arrays pageable, registered (pinned), and registered with the arrays a host sets once declared static.
(The temporaries of `widened` are new arrays of every call: registering the host's float32 arrays does nothing for it.)
Prints one JSON line per (workload, state): minimum and median milliseconds and columns per second of each way.
    --stage     instead: one float32 call per state with the library's stage clock (run with RRTMG_LW_STAGE_TIMING=1; it prints to stderr)
    --kernels   instead: the event time of k_widen_rows and k_narrow_rows in a float32 call (registered arrays) against the library's
                calibration copy (rrtmg_lw_hip_calibrate_stream) on the bytes one launch moves
usage: python tools/e2e_timing_r4.py [--ncol 131072] [--nlay 72] [--config cloudy] [--rounds 5] [--warmup 2] [--stage | --kernels]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rrtmg_lw_amd import api
from rrtmg_lw_amd.synth import make_gcm_inputs

STATIC = ("co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr", "tauaer", "emis")
OUTS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
HOST_BATCH = 16384


def arrays_of(*dicts):
    return [v for d in dicts for v in d.values() if isinstance(v, np.ndarray)]


def travelling_values(d, ncol, nlay):
    """float32 values of the inputs that cross to the device in a non-McICA call with inflglw >= 1 (batches of HOST_BATCH columns): the
    rows that are not uniform for a batch; cloud arrays only in the batch's cloudy layers; taucld travels as float64 sums (not counted)"""
    total = 0
    for c0 in range(0, ncol, HOST_BATCH):
        c1 = min(ncol, c0 + HOST_BATCH)
        cloudy = (np.asarray(d["cldfr"])[c0:c1] >= 1e-20).any(axis=0)
        for k, v in d.items():
            if not isinstance(v, np.ndarray) or k == "taucld":
                continue
            rows = v[c0:c1].reshape((c1 - c0, -1), order="F") if v.ndim > 1 else v[c0:c1, None]
            varying = (rows != rows[0]).any(axis=0)
            if k in ("cldfr", "cicewp", "cliqwp", "reice", "reliq"):
                varying &= cloudy
            total += int(varying.sum()) * (c1 - c0)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=131072)
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--config", default="cloudy")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stage", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    n, nlay = args.ncol, args.nlay

    api.rrtmg_lw_ini(1004.0, kdata=api.STANDIN_KDATA, device=0)
    d64 = make_gcm_inputs(n, nlay, args.config, col0=0)
    d32 = {k: np.asfortranarray(v, dtype=np.float32) if isinstance(v, np.ndarray) else v for k, v in d64.items()}
    d64 = {k: np.asfortranarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v for k, v in d32.items()}      # the same values
    out64, out32 = api._out_arrays(n, nlay, d64["idrv"]), api._out_arrays(n, nlay, d64["idrv"], np.float32)
    for v in arrays_of(out64, out32):
        v[...] = 0.0                               # pages touched: persistent arrays

    def widened(call):
        w = {k: np.asfortranarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v for k, v in d32.items()}
        r = call(w, None, None)
        for k in OUTS:
            out32[k][...] = r[k]

    nomcica = lambda d, out, dt: api.rrtmg_lw_from_dict(d, out=out, dtype=dt)
    # (the fused entry's Python wrapper allocates its outputs: the same for all three ways)
    fused = lambda d, out, dt: api.rrtmg_lw_mcica_subcol_from_dict(d, 140, 0, dtype=dt)
    workloads = {"nomcica": nomcica, "fused_mcica": fused}

    def ways(call):
        return {"f64": lambda: call(d64, out64, None), "r4": lambda: call(d32, out32, np.float32), "widened": lambda: widened(call)}

    def set_state(state, on):
        regs = arrays_of(d64, out64, d32, out32)
        stat = [d[k] for d in (d64, d32) for k in STATIC]
        if state in ("pinned", "pinned_static"):
            for v in regs:
                (api.host_register if on else api.host_unregister)(v)
        if state == "pinned_static":
            for v in stat:
                api.host_static(v) if on else api.host_changed(v, keep=False)

    if args.stage:
        for state in ("pageable", "pinned", "pinned_static"):
            set_state(state, True)
            for _ in range(args.warmup + 1):
                print(f"[e2e_timing_r4 stage] {state}: float32 entry, non-McICA", file=sys.stderr, flush=True)
                nomcica(d32, out32, np.float32)
            set_state(state, False)
        api.finalize()
        return

    if args.kernels:
        lib = api.lib()
        lib.rrtmg_lw_hip_calibrate_stream.argtypes = [ctypes.c_longlong]
        assert n % HOST_BATCH == 0, "--kernels counts the bytes of batches of 16 384 columns"
        launches = n // HOST_BATCH
        win = travelling_values(d32, n, nlay)
        wout = sum(out32[k].size for k in OUTS)

        def profiled(fn):
            buf = ctypes.create_string_buffer(1 << 14)
            lib.rrtmg_lw_hip_profile_begin()
            fn()
            lib.rrtmg_lw_hip_profile_end(buf, len(buf))
            return {ln.split()[0]: (int(ln.split()[1]), float(ln.split()[2])) for ln in buf.value.decode().splitlines() if ln.strip()}

        set_state("pinned", True)
        acc = {"k_widen_rows": [], "k_narrow_rows": []}
        copies = {"k_widen_rows": [], "k_narrow_rows": []}
        per_launch = {"k_widen_rows": 12 * win // launches, "k_narrow_rows": 12 * wout // launches}       # 4 + 8 bytes per value
        for r in range(args.warmup + args.rounds):
            rows = profiled(lambda: nomcica(d32, out32, np.float32))
            for k in acc:
                cp = profiled(lambda k=k: lib.rrtmg_lw_hip_calibrate_stream(per_launch[k] // 2))["k_calibrate"][1]
                if r >= args.warmup:
                    assert rows[k][0] == launches, rows
                    acc[k].append(rows[k][1] / launches)
                    copies[k].append(cp)
        set_state("pinned", False)
        for k in acc:
            t, c = float(np.median(acc[k])), float(np.median(copies[k]))
            print(json.dumps(dict(kernel=k, ncol=n, nlay=nlay, launches_per_call=launches, bytes_per_launch=int(per_launch[k]),
                                  median_ms_per_launch=round(t, 4), min_ms=round(min(acc[k]), 4), max_ms=round(max(acc[k]), 4),
                                  gb_per_s=round(per_launch[k] / t / 1e6, 1), copy_median_ms=round(c, 4),
                                  copy_gb_per_s=round(per_launch[k] / c / 1e6, 1), ratio_to_copy=round(t / c, 2))))
        api.finalize()
        return

    for wname, call in workloads.items():
        w = ways(call)
        # the three ways agree before anything is timed: r4 = widened = rounded f64
        ref = call(d64, out64, None)
        got = call(d32, out32, np.float32)
        for k in OUTS:
            assert np.array_equal(got[k], ref[k].astype(np.float32)), (wname, k)
        for state in ("pageable", "pinned", "pinned_static"):
            set_state(state, True)
            ts = {k: [] for k in w}
            for r in range(args.warmup + args.rounds):
                for k, fn in w.items():
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    if r >= args.warmup:
                        ts[k].append(dt)
            set_state(state, False)
            res = dict(workload=wname, config=args.config, columns=n, nlay=nlay, state=state, rounds=args.rounds)
            for k, v in ts.items():
                res[k] = dict(min_ms=round(1e3 * min(v), 2), median_ms=round(1e3 * float(np.median(v)), 2), max_ms=round(1e3 * max(v), 2),
                              columns_per_s=round(n / min(v)))
            print(json.dumps(res), flush=True)
    api.finalize()


if __name__ == "__main__":
    main()
