#!/usr/bin/env python3
"""Two builds of the library in ONE process, taken in turn (as tools/clear_groups_timing.py alternates a switch), so that drift of the box
cancels: ms per device-resident call of the benchmark's field for each, best and spread over the rounds, and whether the outputs are
the same bit for bit.  Each library is loaded through its own copy of rrtmg_lw_amd.api and keeps its own state and workspace.
Both libraries' streams then share the process's hardware queues: run it in both orders, and do not judge a change of streams or of the
enqueue order by it (profiles/flux_walk.md, section 4).
usage: python tools/ab_libs.py A.so B.so [--config cloudy] [--ncol 1000000] [--nlay 72] [--reps 5] [--rounds 6]"""
import argparse, importlib.util, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs=2)
ap.add_argument("--config", default="cloudy")
ap.add_argument("--ncol", type=int, default=1000000)
ap.add_argument("--nlay", type=int, default=72)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=6)
args = ap.parse_args()
import torch
import rrtmg_lw_amd  # noqa: F401
from rrtmg_lw_amd.synth import make_gcm_inputs
from rrtmg_lw_amd.shard import output_rows, output_views


def load_api(name, lib):
    os.environ["RRTMG_LW_HIP_LIB"] = os.path.abspath(lib)
    spec = importlib.util.spec_from_file_location("rrtmg_lw_amd." + name, os.path.join(ROOT, "rrtmg_lw_amd", "api.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    assert os.path.samefile(mod.LIB_PATH, lib)
    return mod


apis = [load_api("api_a", args.libs[0]), load_api("api_b", args.libs[1])]
dev = torch.device("cuda", 0)
for a in apis:
    a.rrtmg_lw_ini(1004.0, kdata=a.REAL_KDATA if os.path.exists(a.REAL_KDATA) else a.STANDIN_KDATA, device=0)
stream = torch.cuda.current_stream().cuda_stream
slab = 131072
parts = [make_gcm_inputs(min(slab, args.ncol - s), args.nlay, args.config, col0=s, backend="torch", device=dev) for s in range(0, args.ncol, slab)]
d = dict(parts[0])
d["ncol"] = args.ncol
for k, v in parts[0].items():
    if torch.is_tensor(v) and len(parts) > 1:
        cat = torch.cat([p[k] for p in parts], dim=1 if k == "taucld" else 0)
        nd = cat.dim()
        d[k] = cat.permute(*reversed(range(nd))).contiguous().permute(*reversed(range(nd))) if nd > 1 else cat.contiguous()
del parts
idrv = d["idrv"]
bufs = [torch.zeros((output_rows(args.nlay, idrv), args.ncol), dtype=torch.float64, device=dev) for _ in apis]
times = [[] for _ in apis]
for r in range(args.rounds):
    for i, a in enumerate(apis):
        o = output_views(bufs[i], args.nlay, idrv)
        a.rrtmg_lw_device(d, o, stream=stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            a.rrtmg_lw_device(d, o, stream=stream)
        torch.cuda.synchronize()
        times[i].append(1e3 * (time.perf_counter() - t0) / args.reps)
for a in apis:
    a.check(stream)
same = bool(torch.equal(bufs[0].view(torch.int64), bufs[1].view(torch.int64)))
print(f"{args.ncol} '{args.config}' columns x {args.nlay} layers, ms per call, {args.rounds} rounds of {args.reps} calls, A and B in turn")
for nm, lib, t in zip("AB", args.libs, times):
    print(f"  {nm} {lib}: best {min(t):.3f}  spread {max(t) - min(t):.3f}  all " + " ".join(f"{x:.3f}" for x in t))
gap = min(times[0]) - max(times[1])
print(f"  smallest A - B gap (A's best against B's worst) {gap:.3f} ms; larger spread {max(max(t) - min(t) for t in times):.3f} ms; outputs bit-identical: {same}")
for a in apis:
    a.finalize()
