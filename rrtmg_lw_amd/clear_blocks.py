"""What the device decides about clouds per 64-column block, in numpy: the tops k_cloudscan records, the order and hand-off levels k_blocksort
leaves, and k_colsort's order and gain per window of 256 columns (rrtmg_lw_amd/csrc/kernels.hip).  For the tests' premises and
tools/clear_block_stats.py; nothing on the hot path uses it."""
import numpy as np

SORT_GROUP, WIN = 12, 256                   # kernels.hip: blocks per hand-off group, columns of a k_colsort window


def column_tops(cldfr):
    """highest cloudy layer of every column (1 .. nlay; 0: none), k_cloudscan's criterion"""
    c = np.asarray(cldfr) >= 1e-6
    nlay = c.shape[1]
    return np.where(c.any(axis=1), nlay - np.argmax(c[:, ::-1], axis=1), 0)


def block_tops(tops):
    """highest cloudy layer of every block of 64 consecutive positions"""
    t = np.zeros((len(tops) + 63) // 64 * 64, dtype=int)
    t[:len(tops)] = tops
    return t.reshape(-1, 64).max(axis=1)


def sorted_groups(btop):
    """k_blocksort: the blocks by top, deepest first, equal tops in block order; groups of SORT_GROUP consecutive sorted blocks and each
    group's hand-off level, the top of its first block"""
    order = np.argsort(-np.asarray(btop), kind="stable")
    groups = [order[i:i + SORT_GROUP] for i in range(0, len(order), SORT_GROUP)]
    return groups, [int(btop[g[0]]) for g in groups]


def colsort(tops, nlay, min_gain, bonus):
    """k_colsort: per window of 256 columns the order by top (deepest first, equal tops in column order) where its gain reaches min_gain;
    returns (position -> column, every window's gain without the bonus, with it)"""
    perm, gains, gains_b = np.arange(len(tops)), [], []
    for w0 in range(0, len(tops), WIN):
        t = np.full(WIN, -1)
        n = min(WIN, len(tops) - w0)
        t[:n] = tops[w0:w0 + n]
        rank = np.argsort((nlay - t) * WIN + np.arange(WIN), kind="stable")
        nat = np.maximum(t, 0).reshape(-1, 64).max(axis=1)
        srt = np.maximum(t[rank], 0).reshape(-1, 64)[:, 0]
        gain = int((nat - srt).sum())
        gain_b = gain + bonus * int(((srt == 0) & (nat != 0)).sum())
        gains.append(gain)
        gains_b.append(gain_b)
        if gain_b >= min_gain:
            perm[w0:w0 + n] = w0 + rank[:n]
    return perm, gains, gains_b
