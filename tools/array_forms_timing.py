#!/usr/bin/env python3
"""What the *_as device entry costs (include/rrtmg_lw_hip.h, rrtmg_lw_hip_array_form) on the benchmark's call - cloudy 72-layer columns,
rtrnmr - for a torch user who holds float32 (ncol, nlay) tensors with the top of the atmosphere first, form {4, 1, 1}:
  (a) plain    rrtmg_lw_device on reference-form arrays (float64, column fastest, surface first): what the solver itself takes
  (b) as       rrtmg_lw_device(form={4,1,1}) on the user's tensors as they lie
  (c) torch    what such a user does without it: .double(), flip, transpose, .contiguous() on every input, the plain entry, the inverse
               on every output (into preallocated float32 tensors)
The three run interleaved, round by round, in one process; every variant is timed with HIP events on the caller's stream around the
whole step and synchronised.  One JSON line per column count: the median and all rounds of each, the staging bytes per column (growth of
rrtmg_lw_hip_workspace_bytes over the first adapted call), and whether (b) and (c) agree bit for bit.  --kernels adds one more
adapted call under the library's per-kernel event timing (rrtmg_lw_hip_profile_begin / _end): the two conversion kernels' own time.
usage: python tools/array_forms_timing.py [--ncols 1000000,16384] [--nlay 72] [--config cloudy] [--rounds 7] [--kernels]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FLUX = ("uflx", "dflx", "hr", "uflxc", "dflxc", "hrc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncols", default="1000000,16384")
    ap.add_argument("--nlay", type=int, default=72)
    ap.add_argument("--config", default="cloudy")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()

    import torch
    from rrtmg_lw_amd import api, arrays
    from rrtmg_lw_amd.synth import make_gcm_inputs
    if not torch.cuda.is_available():
        sys.exit("array_forms_timing: no GPU - nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    form = arrays.ArrayForm(4, 1, 1)
    nlay = args.nlay
    for ncol in [int(x) for x in args.ncols.split(",")]:
        # (a fresh state per size: the staging figure is the growth over the first adapted call)
        api.rrtmg_lw_ini(1004.0, kdata=api.REAL_KDATA if os.path.exists(api.REAL_KDATA) else api.STANDIN_KDATA, device=0)
        # reference-form inputs, generated in slabs to bound the temporaries (bench.py does the same)
        slab = 131072
        parts = [make_gcm_inputs(min(slab, ncol - s), nlay, args.config, col0=s, backend="torch", device=dev) for s in range(0, ncol, slab)]
        ref = dict(parts[0], ncol=ncol)
        for k, v in parts[0].items():
            if torch.is_tensor(v) and len(parts) > 1:
                ref[k] = torch.cat([p[k] for p in parts], dim=1 if k == "taucld" else 0)
        del parts
        user = arrays.from_reference(ref, form)              # what the torch user holds: float32, (ncol, nlay) contiguous, top first
        ref = arrays.to_reference(user, form)                # ... and the same values in the reference form, for (a)
        names = [k for k in user if torch.is_tensor(user[k])]
        out_ref = arrays.empty_like_form(FLUX, ncol, nlay, arrays.REFERENCE, device=dev)
        out_as = arrays.empty_like_form(FLUX, ncol, nlay, form, device=dev)
        out_torch = arrays.empty_like_form(FLUX, ncol, nlay, form, device=dev)

        def plain():
            api.rrtmg_lw_device(ref, out_ref, stream=stream)

        def adapted():
            api.rrtmg_lw_device(user, out_as, stream=stream, form=form)

        def by_torch():
            d = arrays.to_reference({k: user[k] for k in names}, form)
            d.update({k: v for k, v in user.items() if k not in d})
            o = arrays.empty_like_form(FLUX, ncol, nlay, arrays.REFERENCE, device=dev)
            api.rrtmg_lw_device(d, o, stream=stream)
            back = arrays.from_reference(o, form)
            for k in FLUX:
                out_torch[k].copy_(back[k])

        variants = (("plain", plain), ("as", adapted), ("torch", by_torch))
        plain()
        api.check(stream)
        ws0 = api.workspace_bytes()
        adapted()
        api.check(stream)
        staging = api.workspace_bytes() - ws0
        by_torch()
        api.check(stream)
        same = all(torch.equal(out_as[k], out_torch[k]) for k in FLUX)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {n: [] for n, _ in variants}
        for _ in range(args.rounds):
            for n, f in variants:
                ev[0].record()
                f()
                ev[1].record()
                ev[1].synchronize()
                times[n].append(ev[0].elapsed_time(ev[1]))
        api.check(stream)
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        kernels = None
        if args.kernels:
            api.lib().rrtmg_lw_hip_profile_begin()
            adapted()
            buf = ctypes.create_string_buffer(1 << 16)
            api.lib().rrtmg_lw_hip_profile_end(buf, len(buf))
            kernels = {}
            for line in buf.value.decode().splitlines():
                name, n, ms = line.rsplit(" ", 2)
                kernels[name] = [int(n), round(float(ms), 3)]
        eb = api.effective_batch(nlay)
        nbatch = -(-ncol // eb)
        batch = ncol if nbatch == 1 else min(eb, -(-(-(-ncol // nbatch)) // 256) * 256)        # the library's balanced batch
        print(json.dumps(dict(config=args.config, ncol=ncol, nlay=nlay, form=list(form), rounds=args.rounds,
                              ms={n: round(v, 3) for n, v in med.items()},
                              rounds_ms={n: [round(x, 3) for x in t] for n, t in times.items()},
                              as_minus_plain_ms=round(med["as"] - med["plain"], 3),
                              as_over_plain=round(med["as"] / med["plain"], 3), torch_over_plain=round(med["torch"] / med["plain"], 3),
                              batch_columns=batch, staging_bytes_per_batch_column=round(staging / batch, 1),
                              staging_bytes=staging, as_equals_torch=bool(same), kernels_launches_ms=kernels)), flush=True)
        del ref, user, out_ref, out_as, out_torch
        torch.cuda.empty_cache()
        api.finalize()


if __name__ == "__main__":
    main()
