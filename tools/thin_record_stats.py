#!/usr/bin/env python3
"""Share of series ("thin", odepth <= 0.06) cells and of quad records that are thin in all 64 columns of a block, for the benchmark's columns
(profiles/sweepc_thin_records.md): from the oracle's gas optical depths on the CPU, odepth = secdiff x taug bracketed by 1.50 <= secdiff <= 1.80.
usage: python tools/thin_record_stats.py"""
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_hip_thin_records as T
from test_hip_spectral import inatm
from oracle.bindings import Oracle
from rrtmg_lw_amd.synth import make_gcm_inputs
o = Oracle()
n = 1024
d = make_gcm_inputs(n, 72, "cloudy", col0=0)
taug = np.stack([o.column(inatm(d, i, 0), icld=0, idrv=0)["taug"] for i in range(n)])
quads = T._quads(140)
for name, f in (("certainly thin (1.80 taug <= 0.06)", 1.80), ("possibly thin (1.50 taug <= 0.06)", 1.50)):
    thin = f * taug <= 0.06
    for lo, hi in ((14, 72), (0, 14)):
        cells = thin[:, lo:hi, :].mean()
        rec = np.array([[thin[b * 64:(b + 1) * 64, lay, g0:g0 + m].all() for b in range(n // 64)] for g0, m in quads for lay in range(lo, hi)])
        print(f"{name}, layers {lo + 1}-{hi}: cells {100 * cells:.1f} %, all-thin (quad, layer, block) records {100 * rec.mean():.1f} %")
    # per band above the clouds
    g0 = 0; per = []
    for b, ng in enumerate(T.NG):
        qs = [(g0 + 4 * i, min(4, ng - 4 * i)) for i in range((ng + 3) // 4)]
        rec = np.array([[thin[k * 64:(k + 1) * 64, lay, a:a + m].all() for k in range(n // 64)] for a, m in qs for lay in range(14, 72)])
        per.append(round(100 * rec.mean()))
        g0 += ng
    print("   per band, all-thin records above layer 14 (%):", per)
    # per band thread and level (all of the band's quads)
    g0 = 0; tot = []
    for b, ng in enumerate(T.NG):
        tot.append(np.array([[thin[k * 64:(k + 1) * 64, lay, g0:g0 + ng].all() for k in range(n // 64)] for lay in range(14, 72)]).mean())
        g0 += ng
    print(f"   (band, layer, block) triples all thin above layer 14: {100 * np.mean(tot):.1f} %")
