#!/usr/bin/env python3
"""What a cloudy field offers the cloud-free sweep of a cloudy call (profiles/clear_groups.md), on the CPU from the cloud fraction alone:
the share of cloud-free columns, of cloud-free 64-column blocks and of cloud-free groups of twelve sorted blocks - as the columns lie and
with every window of 256 columns taken by cloud top - and what k_colsort counts as a window's gain, without and with the bonus per block
that becomes cloud-free.
usage: python tools/clear_block_stats.py [--configs cloudy,cloudy_towers,...] [--ncol 65536] [--nlay 72] [--batch 262144] [--bonus 18] [--min-gain 24]"""
import argparse
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rrtmg_lw_amd.clear_blocks import WIN, block_tops, colsort, column_tops, sorted_groups
from rrtmg_lw_amd.synth import make_gcm_inputs
ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="cloudy,cloudy_towers,cloudy_scatter,cloudy_deep,cloudy_orography")
ap.add_argument("--ncol", type=int, default=65536)
ap.add_argument("--nlay", type=int, default=72)
ap.add_argument("--batch", type=int, default=262144, help="columns per batch: the blocks of a batch are sorted together")
ap.add_argument("--bonus", type=int, default=18, help="per cent of nlay block-levels per block that becomes cloud-free (RRTMG_LW_COLSORT_CLEAR)")
ap.add_argument("--min-gain", type=int, default=24)
args = ap.parse_args()
bonus = args.nlay * args.bonus // 100


def groups_free(tops):
    """(cloud-free blocks, cloud-free sorted groups, blocks, groups) over the batches of the field"""
    fb = fg = nb = ng = 0
    for s in range(0, len(tops), args.batch):
        bt = block_tops(tops[s:s + args.batch])
        _, hand = sorted_groups(bt)
        fb += int((bt == 0).sum()); nb += len(bt)
        fg += sum(h == 0 for h in hand); ng += len(hand)
    return fb, fg, nb, ng


for cfg in args.configs.split(","):
    tops = column_tops(make_gcm_inputs(args.ncol, args.nlay, cfg, col0=0)["cldfr"])
    print(f"{cfg}: {args.ncol} columns of {args.nlay} layers, {100 * (tops == 0).mean():.1f} % cloud-free, mean top {tops[tops > 0].mean():.1f}")
    win_free = np.array([(tops[w:w + WIN] == 0).sum() for w in range(0, len(tops), WIN)])
    print(f"   windows of {WIN} with at least 64 cloud-free columns: {100 * (win_free >= 64).mean():.1f} %")
    for name, mg, bn in (("as the columns lie", 1 << 24, 0), ("every window reordered", 0, 0),
                         (f"threshold {args.min_gain}, no bonus", args.min_gain, 0), (f"threshold {args.min_gain}, bonus {bonus}", args.min_gain, bonus)):
        perm, gains, gains_b = colsort(tops, args.nlay, mg, bn)
        fb, fg, nb, ng = groups_free(tops[perm])
        moved = np.mean([g >= mg for g in gains_b])
        print(f"   {name:34s} windows reordered {100 * moved:5.1f} %   cloud-free blocks {100 * fb / nb:5.1f} %   cloud-free groups {100 * fg / ng:5.1f} %")
    _, gains, gains_b = colsort(tops, args.nlay, 0, bonus)
    g, gb = np.array(gains), np.array(gains_b)
    print(f"   window gain in block-levels: mean {g.mean():.1f} (min {g.min()}, max {g.max()}); with the bonus of {bonus}: mean {gb.mean():.1f} (min {gb.min()}, max {gb.max()})")
