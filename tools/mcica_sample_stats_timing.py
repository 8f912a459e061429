#!/usr/bin/env python3
"""What the sample variance, the device-resident forms of the averaging entry and get_alpha on the device cost (profiles/mcica_sample_stats.md).
Four measurements, each in a fresh child process under its own time limit (a child that fails ends the run); libraries that are compared
live in one process and take turns round by round, as in tools/mcica_samples_timing.py; times are device-event times of whole calls
on the caller's stream, ms per call, best of the rounds and the spread over them.
  paths   rrtmg_lw_hip_run_mcica_samples_device of this tree's library (A) against the PARENT build's (B) on the same tensors: the
          existing path must cost what it cost.  B runs twice per round (B, A, B'): B against B' is the parent's own spread.
  var     the new entry with the three variances (A); what a user did before - the parent's fused entry called nsamp times, torch
          forming the mean and var(unbiased=True) of the stacked samples (B); the new entry without variances (C).
  views   float32, layer-fastest, top-first fields through the new entry (A) against torch conversions around the plain samples entry
          (B); {8, 0, 0, ld = ncol + 5} in place (C) against the contiguous call (D).
  alpha   rrtmg_lw_hip_get_alpha_device_view on device tensors (A) against the host entry on the same columns, its copies included (B).
usage: python tools/mcica_sample_stats_timing.py PARENT.so [--ncol 131072] [--nlay 72] [--nsamp 8] [--alpha-ncol 1000000] [--what paths var views alpha]
                                                 [--reps 3] [--rounds 5] [--limit 280]"""
import argparse, importlib.util, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("--ncol", type=int, default=131072)
ap.add_argument("--nlay", type=int, default=72)
ap.add_argument("--nsamp", type=int, default=8)
ap.add_argument("--alpha-ncol", type=int, default=1000000)
ap.add_argument("--what", nargs="+", default=["paths", "var", "views", "alpha"])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=int, default=280, help="seconds a child may take")
ap.add_argument("--child", default=None)
args = ap.parse_args()
SEED, ICLD = 280, 2

if args.child is None:
    print(f"{args.ncol} 'cloudy' columns x {args.nlay} layers, icld = {ICLD}, nsamp = {args.nsamp}, seedstep = sub-columns of a sample; ms per call, "
          f"best of {args.rounds} rounds of {args.reps} calls (spread over the rounds)")
    sys.stdout.flush()
    for what in args.what:
        cmd = [sys.executable, os.path.abspath(__file__), args.parent, "--child", what, "--ncol", str(args.ncol), "--nlay", str(args.nlay),
               "--nsamp", str(args.nsamp), "--alpha-ncol", str(args.alpha_ncol), "--reps", str(args.reps), "--rounds", str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"{what}: the child ended with {rc}; nothing more is started")
            sys.exit(1)
    sys.exit(0)

import numpy as np
import torch
import rrtmg_lw_amd  # noqa: F401
from rrtmg_lw_amd import arrays
from rrtmg_lw_amd.synth import make_gcm_inputs


def load_api(name, lib):
    os.environ["RRTMG_LW_HIP_LIB"] = os.path.abspath(lib)
    spec = importlib.util.spec_from_file_location("rrtmg_lw_amd." + name, os.path.join(ROOT, "rrtmg_lw_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    assert os.path.samefile(mod.LIB_PATH, lib)
    mod.rrtmg_lw_ini(1004.0, kdata=mod.REAL_KDATA if os.path.exists(mod.REAL_KDATA) else mod.STANDIN_KDATA, device=0)
    return mod


def take_turns(runs):
    """runs: (name, callable) in the order of a round -> {name: [ms per call, one per round]}; every callable has run once before"""
    times = {name: [] for name, _ in runs}
    for _, run in runs:
        run()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, run in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
    return times


def row(label, t):
    return f"| {label} | {min(t):.2f} | {max(t) - min(t):.2f} |"


def same_bits(a, b):
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return bool(torch.equal(a.view(it), b.view(it)))


what, nsamp, ncol, nlay = args.child, args.nsamp, args.ncol, args.nlay
dev = torch.device("cuda", 0)
A = load_api("api_a", os.path.join(ROOT, "rrtmg_lw_amd", "librrtmg_lw_hip.so"))
stream = torch.cuda.current_stream().cuda_stream
step = A.gpoints()
FLUX = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")
VAR = ("uflx_var", "dflx_var", "hr_var")
STAT = ("uflx", "dflx", "hr")
new_out = lambda names, form=arrays.REFERENCE: arrays.empty_like_form(names, ncol, nlay, form, device=dev, fill=float("nan"))
result = {"what": what, "ncol": ncol, "nlay": nlay, "nsamp": nsamp}

if what == "paths":
    B = load_api("api_b", args.parent)
    d = make_gcm_inputs(ncol, nlay, "cloudy", backend="torch", device=dev)
    oa, ob = new_out(FLUX), new_out(FLUX)
    run_a = lambda: A.rrtmg_lw_mcica_subcol_device(d, oa, SEED, 0, icld=ICLD, stream=stream, nsamp=nsamp, seedstep=step)
    run_b = lambda: B.rrtmg_lw_mcica_subcol_device(d, ob, SEED, 0, icld=ICLD, stream=stream, nsamp=nsamp, seedstep=step)
    t = take_turns([("B", run_b), ("A", run_a), ("B'", run_b)])
    A.check(stream); B.check(stream)
    same = all(same_bits(oa[k], ob[k]) for k in FLUX)
    print("\n### paths: rrtmg_lw_hip_run_mcica_samples_device, this tree (A) and the parent build (B, B': twice per round)\n")
    print("| library | ms per call | spread |\n|---|---|---|")
    for k in ("A", "B", "B'"):
        print(row(k, t[k]))
    per_round = [abs(x - y) for x, y in zip(t["B"], t["B'"])]
    best_a, best_b, best_b2 = min(t["A"]), min(t["B"]), min(t["B'"])
    print(f"\nA - B = {best_a - best_b:+.2f} ms; the parent against itself within a round: up to {max(per_round):.2f} ms, "
          f"best B' - best B = {best_b2 - best_b:+.2f} ms.  Outputs bit-identical: {same}")
    result.update(times=t, bit_identical=same)
    B.finalize()
elif what == "var":
    B = load_api("api_b", args.parent)
    d = make_gcm_inputs(ncol, nlay, "cloudy", backend="torch", device=dev)
    oa, oc, tmp = new_out(FLUX + VAR), new_out(FLUX), new_out(FLUX)
    stack = {k: torch.empty((nsamp,) + tuple(oc[k].shape), dtype=torch.float64, device=dev) for k in STAT}
    ob = {}

    def run_a():
        A.rrtmg_lw_mcica_samples_device(d, oa, SEED, nsamp, seedstep=step, icld=ICLD, stream=stream)

    def run_c():
        A.rrtmg_lw_mcica_samples_device(d, oc, SEED, nsamp, seedstep=step, icld=ICLD, stream=stream)

    def run_b():
        for s in range(nsamp):
            B.rrtmg_lw_mcica_subcol_device(d, tmp, SEED + s * step, 0, icld=ICLD, stream=stream)
            for k in STAT:
                stack[k][s].copy_(tmp[k])
        for k in STAT:
            ob[k + "_var"], ob[k] = torch.var_mean(stack[k], dim=0, unbiased=True)

    t = take_turns([("A", run_a), ("B", run_b), ("C", run_c)])
    A.check(stream); B.check(stream)
    mean_same = all(same_bits(oa[k], oc[k]) for k in FLUX)
    rel = max(float(((oa[k + "_var"] - ob[k + "_var"]).abs() / ob[k + "_var"].clamp_min(1e-6)).max()) for k in STAT)
    print("\n### var: the three variances\n")
    print("| what | ms per call | spread |\n|---|---|---|")
    print(row("A: new entry, uflx_var + dflx_var + hr_var", t["A"]))
    print(row("B: parent's fused entry x nsamp, torch.var_mean of the stacked samples", t["B"]))
    print(row("C: new entry, no variances", t["C"]))
    print(f"\nA / B = {min(t['A']) / min(t['B']):.3f}; the statistics cost A - C = {min(t['A']) - min(t['C']):+.2f} ms "
          f"({100 * (min(t['A']) / min(t['C']) - 1):+.1f} %).  Means of A and C bit-identical: {mean_same}; A's variances against torch's: "
          f"max relative difference {rel:.1e} (where var > 1e-6)")
    result.update(times=t, mean_bit_identical=mean_same, var_rel=rel)
    B.finalize()
elif what == "views":
    form = arrays.ArrayForm(4, 1, 1)
    dn = make_gcm_inputs(ncol, nlay, "cloudy")
    x = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in arrays.from_reference(dn, form).items()}
    ref = {k: (torch.from_numpy(np.asfortranarray(v) if v.ndim > 1 else v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in dn.items()}
    oa = new_out(FLUX + VAR, form)
    oplain = new_out(FLUX)
    ob = {}

    def run_a():
        A.rrtmg_lw_mcica_samples_device(x, oa, SEED, nsamp, seedstep=step, icld=ICLD, stream=stream, form=form)

    def run_b():       # what such a host does without the entry: widen and transpose with torch, call the plain entry, convert back (means only)
        w = arrays.to_reference(x, form)
        A.rrtmg_lw_mcica_subcol_device(w, oplain, SEED, 0, icld=ICLD, stream=stream, nsamp=nsamp, seedstep=step)
        ob.update(arrays.from_reference(oplain, form))

    ld = ncol + 5
    emb = {k: arrays.embed(v, k, arrays.REFERENCE, ld, 0)[1] for k, v in ref.items() if torch.is_tensor(v)}
    dv = dict(ref, **emb)
    ov = {k: arrays.embed(v, k, arrays.REFERENCE, ld, 0)[1] for k, v in new_out(FLUX + VAR).items()}
    od = new_out(FLUX + VAR)
    run_c = lambda: A.rrtmg_lw_mcica_samples_device(dv, ov, SEED, nsamp, seedstep=step, icld=ICLD, stream=stream, ld=ld)
    run_d = lambda: A.rrtmg_lw_mcica_samples_device(ref, od, SEED, nsamp, seedstep=step, icld=ICLD, stream=stream)
    t = take_turns([("A", run_a), ("B", run_b), ("C", run_c), ("D", run_d)])
    A.check(stream)
    same_ab = all(same_bits(oa[k], ob[k]) for k in FLUX)
    same_cd = all(same_bits(ov[k].contiguous(), od[k].contiguous()) for k in FLUX + VAR)
    print("\n### views\n")
    print("| what | ms per call | spread |\n|---|---|---|")
    print(row("A: float32 layer-fastest top-first fields, new entry with variances", t["A"]))
    print(row("B: the same fields, torch conversions around the plain samples entry (no variances)", t["B"]))
    print(row(f"C: float64 fields ld = ncol + 5 wide, in place, with variances", t["C"]))
    print(row("D: contiguous float64 tensors, with variances", t["D"]))
    print(f"\nA / B = {min(t['A']) / min(t['B']):.3f}, C - D = {min(t['C']) - min(t['D']):+.2f} ms.  A's means equal B's bit for bit: {same_ab}; "
          f"C equals D bit for bit: {same_cd}")
    result.update(times=t, ab_bit_identical=same_ab, cd_bit_identical=same_cd)
elif what == "alpha":
    n = args.alpha_ncol
    rng = np.random.default_rng(3)
    g = {"ncol": n, "nlay": nlay, "dz": np.asfortranarray(rng.uniform(100, 1500, (n, nlay))), "lat": rng.uniform(-90, 90, n),
         "cldfr": np.asfortranarray(make_gcm_inputs(n, nlay, "cloudy")["cldfr"])}
    gd = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    alpha = arrays.empty_like_form(("alpha",), n, nlay, arrays.REFERENCE, device=dev, fill=float("nan"))["alpha"]
    run_a = lambda: A.get_alpha_device(gd, alpha, 5, 1, 2000.0, 100, stream=stream)
    t = take_turns([("A", run_a)])
    A.check(stream)
    host, wall = None, []
    for r in range(args.rounds):
        t0 = time.perf_counter()
        host = A.get_alpha(n, nlay, 5, 1, 2000.0, g["dz"], g["lat"], 100, g["cldfr"])
        wall.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(alpha.cpu().numpy(), host))
    print(f"\n### alpha: {n} columns x {nlay} layers, icld = 5, idcor = 1\n")
    print("| what | ms per call | spread |\n|---|---|---|")
    print(row("A: rrtmg_lw_hip_get_alpha_device_view, device tensors (device-event time)", t["A"]))
    print(row("B: rrtmg_lw_hip_get_alpha, host arrays, its copies included (wall time)", wall))
    print(f"\nbit-identical: {same}")
    result.update(ncol=n, times=t, host_ms=wall, bit_identical=same)
else:
    raise SystemExit(f"unknown measurement {what}")
print("# " + json.dumps(result), flush=True)
A.finalize()
