#!/usr/bin/env python3
"""MTF ranks of the run heads of the bench text, laid out as mtf_replay walks them (CPU only, oracle RLE1 + BWT).

usage: tools/mtf_rank_tiers.py [MB of the bench input, default 10] [level, default 9]

mtf_replay gives one lane to each chunk of 512 run heads: chunk c of a block is lane c mod 64 of wave c div 64, and step t
of a wave replays head t of each of its 64 chunks.  A wave has to walk the list as far as its deepest lane, so what prices
a step is the MAXIMUM rank over the lanes.  Prints (a) the histogram of the ranks, (b) the histogram of that maximum per wave
step, and what (b) means in list words walked per step (4 positions per word, 16 words in registers) for some tier widths.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recipes  # noqa: E402
import support  # noqa: E402

CHUNK, LANES, RW = 512, 64, 16
EDGES = [4, 8, 16, 32, 64]
NAMES = ["<4", "<8", "<16", "<32", "<64", ">=64"]


def head_ranks(U):
    """MTF ranks of the run heads of U (inside a run the rank is 0 and the list does not move)"""
    heads = U[np.concatenate(([True], U[1:] != U[:-1]))]
    lst = sorted(set(heads.tolist()))
    out = np.empty(heads.size, dtype=np.int32)
    for i, s in enumerate(heads.tolist()):
        r = lst.index(s)
        out[i] = r
        if r:
            lst.insert(0, lst.pop(r))
    return out


def wave_step_max(ranks):
    """max rank over the 64 lanes for every step of every wave of one block (lanes past the last head take no part)"""
    nch = -(-ranks.size // CHUNK)
    nw = -(-nch // LANES)
    grid = np.full(nw * LANES * CHUNK, -1, dtype=np.int32)
    grid[:ranks.size] = ranks
    m = grid.reshape(nw, LANES, CHUNK).max(axis=1).ravel()       # [wave][step]
    return m[m >= 0]


def bucket(v):
    h = np.bincount(np.searchsorted(EDGES, v, side="right"), minlength=6)
    return h


def tiers_words(m, tiers):
    """list words a wave step walks under tier bounds `tiers` (cumulative word counts), search and shift alike"""
    need = np.minimum(m, 4 * RW - 1) // 4 + 1
    b = np.asarray(tiers)
    return b[np.searchsorted(b, need, side="left")]


def main():
    mb = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    level = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    data = recipes.textgen(mb * 1000000, 1)
    orc = support.Oracle()
    blocks = orc.rle1_blocks(data, level)
    allr, allm, nheads = [], [], 0
    for blk, _, _, _ in blocks:
        U, _ = orc.bwt_cyclic(blk)
        r = head_ranks(U)
        nheads += r.size
        allr.append(r)
        allm.append(wave_step_max(r))
    r = np.concatenate(allr)
    m = np.concatenate(allm)
    print("input: textgen(%d, 1), level %d: %d blocks, %d run heads (%.3f per byte), %d wave steps" %
          (data.size, level, len(blocks), nheads, nheads / data.size, m.size))
    print("(a) ranks of the heads                      (b) max rank over the 64 lanes of a wave step")
    ha, hb = bucket(r), bucket(m)
    ca, cb = np.cumsum(ha) / r.size, np.cumsum(hb) / m.size
    for k in range(6):
        print("  %-5s %10d  %6.2f %%  cum %6.2f %%        %-5s %9d  %6.2f %%  cum %6.2f %%" %
              (NAMES[k], ha[k], 100.0 * ha[k] / r.size, 100 * ca[k], NAMES[k], hb[k], 100.0 * hb[k] / m.size, 100 * cb[k]))
    print("mean rank %.2f, mean of the wave-step maximum %.2f" % (r.mean(), m.mean()))
    need = np.minimum(m, 4 * RW - 1) // 4 + 1
    print("words a wave step needs (max rank / 4 + 1, at most 16): mean %.2f of 16" % need.mean())
    print("  needed words:", " ".join("%d:%.1f%%" % (k, 100.0 * np.mean(need == k)) for k in range(1, RW + 1)))
    for tiers in ([16], [4, 8, 16], [2, 4, 8, 16], [4, 16], [8, 16], [2, 4, 6, 8, 12, 16], list(range(1, 17))):
        w = tiers_words(m, tiers).mean()
        print("  tiers ending at words %-22s mean words walked %5.2f = %4.1f %% of 16" % (tiers, w, 100 * w / RW))


if __name__ == "__main__":
    main()
