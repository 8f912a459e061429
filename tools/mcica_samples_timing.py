#!/usr/bin/env python3
"""The mean over nsamp sub-column samples, device-resident: A = rrtmg_lw_hip_run_mcica_samples_device of this tree's library against
B = the existing fused device entry of ANOTHER build of the library (the parent commit's), called nsamp times with the seeds and
accumulated with in-place torch adds and one division.  Both libraries live in one process and take turns, round by round (as
tools/ab_libs.py does), so that drift of the box cancels; times are device-event times of whole calls on the caller's stream.
Per nsamp one fresh child process under its own time limit; a child that fails ends the run.  Prints a markdown table row per nsamp:
ms per call for A and B (best of the rounds, and the spread over them), the library's device memory after A, whether A's outputs
equal B's bit for bit.
usage: python tools/mcica_samples_timing.py PARENT.so [--ncol 131072] [--nlay 72] [--nsamp 1 2 4 8 16] [--reps 3] [--rounds 5] [--limit 240]"""
import argparse, importlib.util, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("--ncol", type=int, default=131072)
ap.add_argument("--nlay", type=int, default=72)
ap.add_argument("--nsamp", type=int, nargs="+", default=[1, 2, 4, 8, 16])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
ap.add_argument("--child", action="store_true")
args = ap.parse_args()
SEED, ICLD = 280, 2
TOTAL = ("uflx", "dflx", "hr")
KEYS = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")

if not args.child:
    print(f"{args.ncol} 'cloudy' columns x {args.nlay} layers, icld = {ICLD}, irng = 0, seedstep = sub-columns of a sample; ms per call, "
          f"best of {args.rounds} rounds of {args.reps} calls (spread over the rounds), A and B in turn")
    print("| nsamp | A: samples entry | B: parent, nsamp calls + torch | A / B | workspace after A (MB) | bit-identical |")
    print("|---|---|---|---|---|---|")
    sys.stdout.flush()
    for n in args.nsamp:
        cmd = [sys.executable, os.path.abspath(__file__), args.parent, "--child", "--ncol", str(args.ncol), "--nlay", str(args.nlay),
               "--nsamp", str(n), "--reps", str(args.reps), "--rounds", str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"nsamp = {n}: the child ended with {rc}; nothing more is started")
            sys.exit(1)
    sys.exit(0)

import torch
import rrtmg_lw_amd  # noqa: F401
from rrtmg_lw_amd.synth import make_gcm_inputs


def load_api(name, lib):
    os.environ["RRTMG_LW_HIP_LIB"] = os.path.abspath(lib)
    spec = importlib.util.spec_from_file_location("rrtmg_lw_amd." + name, os.path.join(ROOT, "rrtmg_lw_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    assert os.path.samefile(mod.LIB_PATH, lib)
    return mod


nsamp = args.nsamp[0]
A = load_api("api_a", os.path.join(ROOT, "rrtmg_lw_amd", "librrtmg_lw_hip.so"))
B = load_api("api_b", args.parent)
dev = torch.device("cuda", 0)
for a in (A, B):
    a.rrtmg_lw_ini(1004.0, kdata=a.REAL_KDATA if os.path.exists(a.REAL_KDATA) else a.STANDIN_KDATA, device=0)
step = A.gpoints()
stream = torch.cuda.current_stream().cuda_stream
d = make_gcm_inputs(args.ncol, args.nlay, "cloudy", backend="torch", device=dev)
assert d["idrv"] == 0


def outputs():
    o = {k: torch.full((args.nlay + 1, args.ncol), float("nan"), dtype=torch.float64, device=dev) for k in ("uflx", "dflx", "uflxc", "dflxc")}
    o.update({k: torch.full((args.nlay, args.ncol), float("nan"), dtype=torch.float64, device=dev) for k in ("hr", "hrc")})
    return o


oa, ob, tmp = outputs(), outputs(), outputs()
div = torch.tensor([float(nsamp)], dtype=torch.float64, device=dev)          # (a tensor: torch divides by it, it does not multiply by 1 / nsamp)


def run_a():
    A.rrtmg_lw_mcica_subcol_device(d, oa, SEED, 0, icld=ICLD, stream=stream, nsamp=nsamp, seedstep=step)


def run_b():
    B.rrtmg_lw_mcica_subcol_device(d, ob, SEED, 0, icld=ICLD, stream=stream)
    for s in range(1, nsamp):
        B.rrtmg_lw_mcica_subcol_device(d, tmp, SEED + s * step, 0, icld=ICLD, stream=stream)
        for k in TOTAL:
            ob[k].add_(tmp[k])
    if nsamp > 1:
        for k in TOTAL:
            ob[k].div_(div)


times = {"A": [], "B": []}
for name, run in (("A", run_a), ("B", run_b)):
    run()
torch.cuda.synchronize()
for r in range(args.rounds):
    for name, run in (("A", run_a), ("B", run_b)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.reps)
A.check(stream)
B.check(stream)
same = all(bool(torch.equal(oa[k].view(torch.int64), ob[k].view(torch.int64))) for k in KEYS)
ws = A.workspace_bytes()
ta, tb = times["A"], times["B"]
print(f"| {nsamp} | {min(ta):.2f} ({max(ta) - min(ta):.2f}) | {min(tb):.2f} ({max(tb) - min(tb):.2f}) | {min(ta) / min(tb):.3f} | {ws / 1e6:.0f} | {same} |")
print("# " + json.dumps({"nsamp": nsamp, "ncol": args.ncol, "nlay": args.nlay, "A_ms": ta, "B_ms": tb, "workspace_bytes": ws, "bit_identical": same,
                         "kiss_tables_built": A.kiss_tables_built()}), flush=True)
for a in (A, B):
    a.finalize()
