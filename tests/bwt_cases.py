"""Inputs of the suffix sort's stage tests that more than one test file builds (test_gpu_bwt_flags.py through cjs_stage_bwt, the
fixed geometry; test_gpu_bwt_var.py through cjs_stage_bwt_var, blocks of different lengths in slots of one stride), and the CPU
model of round 1 that shows where their groups land.  No GPU and no product code in here."""
import numpy as np

import recipes

WIN = 3072          # nominal range of a tile-sorter window (TS_NOM in bwt_rules.h): a window owns the groups that start in it


# ---- planted groups at chosen places of the compacted array ---------------------------------------------------------------
# Background and filling bytes are random in [0x40, 0x80): with 64^7 possible 7-grams next to nothing of it repeats, so round 1
# (depth 7) resolves it.  A planted unit starts with a two-byte id (first byte below 0x40, second at or above 0x80) and occurs
# m times: its occurrences are a group of m suffixes after round 1, the groups of all units come FIRST in the compacted array
# (their first byte sorts below everything else) and in id order.  So the array that round 2 sorts starts with groups of exactly
# the sizes planted, in the order planted, and a group's start slot is the sum of the sizes in front of it.  (The suffixes one
# byte into a unit repeat six of its bytes, and the few that also agree in the byte behind form small groups of their own:
# those start with a byte >= 0x40 and sort behind all planted groups.)  A size of 1 cannot be planted: a suffix alone in its
# group is resolved and leaves the array; every case makes thousands of them as NEW groups.
# The filler groups between the targets decide which tile sorter round 2 takes (radix_tile_sorter in bwt_rules.h: the LDS radix
# sorter from 5 suffixes per group on, the counting / bitonic sorter below): fillers of 450 put the targets through
# bwt_tile_sort_radix, fillers of 2 and 3 through bwt_tile_sort.  Those take more units than two id bytes number (64 * 128): a
# third id byte, again at or above 0x80, keeps "first byte below 0x40, in id order".
def planted(sizes_and_offsets, unit_len, sep_len, seed, tiny_fillers=False):
    """sizes_and_offsets: [(group size, offset of its first slot from a multiple of WIN)] -> (bytes, [(start slot, size)])"""
    rng = np.random.default_rng(seed)
    plan = []                      # sizes of all planted groups in array order
    targets = []
    at = 0

    def fill(gap):
        nonlocal at
        if tiny_fillers and gap:
            assert gap >= 2
            while gap > 4:         # 2, 3, 2, 3, ... and a rest of 2, 3 or 2 + 2
                m = 2 + (len(plan) & 1)
                plan.append(m); gap -= m; at += m
            for m in ((2, 2) if gap == 4 else (gap,)):
                plan.append(m); at += m
            return
        while gap > 900:
            plan.append(450); gap -= 450; at += 450
        if gap:
            assert gap >= 2
            plan.append(gap); at += gap

    for size, off in sizes_and_offsets:
        want = (at // WIN + 1) * WIN + off
        while want - at < 2 and want != at:
            want += WIN
        fill(want - at)
        targets.append((at, size))
        plan.append(size); at += size
    fill(5)                        # the last target is not the end of the planted part
    parts = []
    for uid, m in enumerate(plan):
        unit = rng.integers(0x40, 0x80, unit_len, dtype=np.uint8)
        if tiny_fillers:
            unit[0] = uid >> 14; unit[1] = 0x80 | ((uid >> 7) & 127); unit[2] = 0x80 | (uid & 127)
            assert uid < 64 * 128 * 128
        else:
            unit[0] = uid >> 7; unit[1] = 0x80 | (uid & 127)
            assert uid < 64 * 128
        occ = rng.integers(0x40, 0x80, (m, unit_len + sep_len), dtype=np.uint8)
        occ[:, :unit_len] = unit
        parts.append(occ.reshape(-1))
    data = np.concatenate(parts)
    # occurrences of one unit stand apart: shuffle all occurrences (same length each) so that no unit is periodic in the text
    occs = data.reshape(-1, unit_len + sep_len)
    data = occs[rng.permutation(occs.shape[0])].reshape(-1)
    return np.ascontiguousarray(data), targets


SIZES = (2, 64, 65, 1023, 1024, 1025)
SHALLOW = [(s, o) for s in SIZES for o in (-1, 0, 1)]        # unit of 7 bytes: the groups split into singletons in round 2
DEEP = [(s, o) for s in (65, 1024, 1025) for o in (-1, 0, 1)]  # unit of 15 bytes: they pass round 2 whole (1025: deferred twice) and split in round 3
PLANTED = {
    "shallow": lambda: planted(SHALLOW, 7, 5, 101),
    "deep": lambda: planted(DEEP, 15, 4, 102),
    "tiny": lambda: planted(SHALLOW, 7, 5, 103, tiny_fillers=True),      # the shallow targets among fillers of 2 and 3
}


def round1_depth_var(nb):
    """symbols of the round-1 key over nb blocks of different lengths: round1_keys(nb, true, false, true).nsym in bwt_rules.h
    (the block id and the hole bit share the 64 bits with the 8-bit symbols; tests/host/bwt_rules_check.cc pins the same
    thresholds on the header)"""
    return min(7, (64 - ((nb - 1).bit_length() + 1)) // 8)


def groups_after_round1(blocks, d=7):
    """(start slot, size) of the groups of the compacted array after a cyclic round of depth d over `blocks` (a list of byte
    arrays), in array order: block by block, inside a block by the d leading symbols of each rotation, which wrap at the block's
    own length (more than once in a block shorter than d)"""
    lens = np.array([b.size for b in blocks], dtype=np.int64)
    assert lens.size and lens.min() >= 1 and 1 <= d <= 7
    flat = np.concatenate(blocks).astype(np.uint64)
    start = np.repeat(np.cumsum(lens) - lens, lens)
    n = np.repeat(lens, lens)
    i = np.arange(flat.size, dtype=np.int64) - start
    key = np.zeros(flat.size, dtype=np.uint64)
    for j in range(d):
        key = (key << np.uint64(8)) | flat[start + (i + j) % n]
    blk = np.repeat(np.arange(lens.size, dtype=np.uint64), lens)
    if (lens.size - 1).bit_length() + 8 * d <= 64:
        key |= blk << np.uint64(8 * d)
        key.sort()
        head = np.concatenate([[True], key[1:] != key[:-1]])
    else:
        order = np.lexsort((key, blk))
        key, blk = key[order], blk[order]
        head = np.concatenate([[True], (key[1:] != key[:-1]) | (blk[1:] != blk[:-1])])
    starts = np.flatnonzero(head)
    sizes = np.diff(np.concatenate([starts, [flat.size]]))
    sizes = sizes[sizes > 1]
    return list(zip((np.cumsum(sizes) - sizes).tolist(), sizes.tolist()))


# ---- equal rank keys inside a group ----------------------------------------------------------------------------------------
def pages(page_len, copies, seed):
    """a page repeated `copies` times, each copy followed by one byte of its own: the suffixes at one page offset form a group
    whose members carry EQUAL rank keys round after round (the next difference is up to page_len bytes away), so they must stay
    one group with one new head; 40 copies take the counting path of the tile sorter, 70 and 300 the bitonic / radix paths"""
    page = recipes.textgen(page_len, seed)
    return np.concatenate([np.concatenate([page, np.array([48 + i % 200], dtype=np.uint8)]) for i in range(copies)])


EQUAL_KEY_INPUTS = {
    "pages_40x5000": lambda: pages(5000, 40, 21),
    "pages_70x5000": lambda: pages(5000, 70, 22),
    "pages_300x1500": lambda: pages(1500, 300, 23),
}


# ---- groups of more than 1024 suffixes in rounds > 2, and the whole-array fallbacks -------------------------------------------
# name -> (bytes, block length)
FALLBACK_INPUTS = {
    # periodic stretches inside text with periods that are no powers of two: groups of ~16,000 and ~28,000 suffixes that go
    # through compact -> radix passes -> bwt_defer_scatter for a dozen rounds, with text groups in the tile sorters beside them
    "text_plus_period12": lambda: (recipes.build({"kind": "concat", "parts": [
        {"kind": "textgen", "n": 500000, "seed": 31}, {"kind": "repeat", "unit_hex": "6162636465666768696a6b6c", "n": 200000},
        {"kind": "textgen", "n": 99981, "seed": 32}]}), 799981),
    "text_plus_period7": lambda: (recipes.build({"kind": "concat", "parts": [
        {"kind": "textgen", "n": 300000, "seed": 33}, {"kind": "repeat", "unit_hex": "71727374757677", "n": 200003},
        {"kind": "textgen", "n": 50000, "seed": 34}]}), 550003),
    # more than half of the workspace deferred: the whole array is sorted by keys that are gathered again (bwt_key_flags)
    "zeros_900k": lambda: (np.zeros(900000, dtype=np.uint8), 900000),
    "period2_900k": lambda: (recipes.build({"kind": "repeat", "unit_hex": "6162", "n": 900000}), 900000),
    # fewer than 8192 unresolved suffixes from the start, or falling below that on the way: whole-array radix passes
    "repeats_5k": lambda: (np.tile(recipes.textgen(1700, 41), 3)[:5000].copy(), 5000),
    "repeats_7k": lambda: (np.tile(recipes.textgen(900, 42), 8)[:7000].copy(), 7000),
    "repeats_9k": lambda: (np.tile(recipes.textgen(2900, 43), 4)[:9000].copy(), 9000),
    "repeats_9k_two_blocks": lambda: (np.tile(recipes.textgen(2100, 44), 9)[:18000].copy(), 9000),
}
