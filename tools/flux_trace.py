#!/usr/bin/env python3
"""Reads a rocprofv3 kernel-trace CSV of the benchmark (per-dispatch start, end, queue id; no counters, no other tracing domain) and says
what runs beside k_flux (profiles/flux_walk.md): per k_flux dispatch its batch of the step, its duration and the dispatches that overlap
it; per batch of the step the mean / minimum / maximum duration and the overlap per kernel family; the hardware queues the process used and
which kernel families each carried.
usage: python tools/flux_trace.py kernel_trace.csv [--batches 4] [--skip-steps 3] [--list 8]"""
import argparse, csv, re
ap = argparse.ArgumentParser()
ap.add_argument("csv")
ap.add_argument("--batches", type=int, default=4, help="k_flux launches per step")
ap.add_argument("--skip-steps", type=int, default=3, help="warm-up steps left out of the statistics")
ap.add_argument("--list", type=int, default=8, help="k_flux dispatches listed one by one (the last ones)")
args = ap.parse_args()


def family(nm):
    m = re.search(r"(k_\w+)(<[^>(]*>)?", nm)
    return (m.group(1) + (m.group(2) or "")) if m else nm[:40]


ev = []
for r in csv.DictReader(open(args.csv)):
    nm = r.get("Kernel_Name") or r.get("Name")
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), family(nm), r.get("Queue_Id", "?")))
ev.sort()
queues = {}
for s, e, f, q in ev:
    queues.setdefault(q, {}).setdefault(f.split("<")[0], 0)
    queues[q][f.split("<")[0]] += 1
print(f"{len(ev)} dispatches on {len(queues)} hardware queues")
for q, fams in sorted(queues.items()):
    print(f"  queue {q}: " + ", ".join(f"{f} x{n}" for f, n in sorted(fams.items())))

flux = [i for i, x in enumerate(ev) if x[2].startswith("k_flux")]
flux = flux[args.skip_steps * args.batches:]
per = [dict(d=[], ov={}) for _ in range(args.batches)]
lines = []
for n, i in enumerate(flux):
    s, e, f, q = ev[i]
    b = n % args.batches
    per[b]["d"].append(e - s)
    beside = []
    j = i - 1
    while j >= 0 and ev[j][0] > s - 200_000_000:        # (sorted by start: look back 200 ms, ahead until a start past the end)
        if ev[j][1] > s: beside.append(j)
        j -= 1
    j = i + 1
    while j < len(ev) and ev[j][0] < e:
        beside.append(j)
        j += 1
    txt = []
    for j in sorted(beside):
        s2, e2, f2, q2 = ev[j]
        o = min(e, e2) - max(s, s2)
        per[b]["ov"][f2] = per[b]["ov"].get(f2, 0) + o
        txt.append(f"{f2} q{q2} {o / 1e3:.0f} us of its {(e2 - s2) / 1e3:.0f}")
    lines.append(f"  batch {b} q{q} {(e - s) / 1e3:7.1f} us   beside: " + ("; ".join(txt) if txt else "nothing"))
print(f"\nk_flux per batch of the step ({len(flux) // args.batches} steps):")
print("| batch | launches | mean us | min | max | overlapped by (mean us per launch) |\n|---|---|---|---|---|---|")
for b, p in enumerate(per):
    if not p["d"]: continue
    n = len(p["d"])
    ov = ", ".join(f"{f} {t / n / 1e3:.0f}" for f, t in sorted(p["ov"].items(), key=lambda kv: -kv[1])) or "nothing"
    print(f"| {b} | {n} | {sum(p['d']) / n / 1e3:.1f} | {min(p['d']) / 1e3:.1f} | {max(p['d']) / 1e3:.1f} | {ov} |")
alld = [x for p in per for x in p["d"]]
if alld:
    print(f"all: {len(alld)} launches, mean {sum(alld) / len(alld) / 1e3:.1f} us, min {min(alld) / 1e3:.1f}, max {max(alld) / 1e3:.1f}")
print(f"\nthe last {args.list} k_flux dispatches:")
print("\n".join(lines[-args.list:]))
