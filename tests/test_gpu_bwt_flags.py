"""Suffix sort rounds >= 2 with head flags as bytes (bwt_tile_sort.hip, bwt_defer.hip, bwt_regroup.hip: hflag[]): inputs aimed at the seams of that form.

Rounds >= 2 no longer pass a sorted 64-bit key per slot from the sorters to the regroup kernels but one flag byte (bit 0 = head
of the new grouping, bit 1 = head of the previous round's grouping).  Every slot has one writer: the tile-sorter window that
owns its group, bwt_defer_scatter (groups of more than 1024 suffixes), or bwt_key_flags behind the whole-array fallbacks.
The cases below put groups on the borders between those writers.  All of them compare block by block with the oracle's BWT
through cjs_stage_bwt, in both forms (cyclic = bzip2, sentinel = BWTC).
The last test sorts round 1 unsegmented; its second input is long enough for the radix sorter (radix.hip) to scan the tile
counts of its one segment in three kernels instead of one.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import recipes
import support

ROOT = support.ROOT
WIN = 3072          # nominal range of a tile-sorter window (TS_NOM in bwt_rules.h): a window owns the groups that start in it


def _check_bwt(hip, oracle, data, block_len, cyclic):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    rc, U, pidx = hip.stage_bwt(data, block_len, cyclic)
    assert rc == 0
    nb = -(-data.size // block_len)
    for k in range(nb):
        blk = data[k * block_len:(k + 1) * block_len]
        eu, ep = (oracle.bwt_cyclic if cyclic else oracle.bwt_sentinel)(blk)
        got = U[k * block_len:k * block_len + blk.size]
        assert pidx[k] == ep, "pidx block %d: got %d want %d (n=%d cyclic=%s)" % (k, pidx[k], ep, blk.size, cyclic)
        if not np.array_equal(got, eu):
            bad = np.nonzero(got != eu)[0]
            raise AssertionError("BWT bytes differ in block %d at %d positions, first %d (n=%d cyclic=%s)" % (k, bad.size, bad[0], blk.size, cyclic))


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
def _planted(sizes_and_offsets, unit_len, sep_len, seed, tiny_fillers=False):
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


_SIZES = (2, 64, 65, 1023, 1024, 1025)
_SHALLOW = [(s, o) for s in _SIZES for o in (-1, 0, 1)]        # unit of 7 bytes: the groups split into singletons in round 2
_DEEP = [(s, o) for s in (65, 1024, 1025) for o in (-1, 0, 1)]  # unit of 15 bytes: they pass round 2 whole (1025: deferred twice) and split in round 3
_PLANTED = {
    "shallow": lambda: _planted(_SHALLOW, 7, 5, 101),
    "deep": lambda: _planted(_DEEP, 15, 4, 102),
    "tiny": lambda: _planted(_SHALLOW, 7, 5, 103, tiny_fillers=True),      # the shallow targets among fillers of 2 and 3
}


def _groups_after_round1(data):
    """(start slot, size) of the groups of the compacted array after a depth-7 cyclic round, in array order"""
    n = data.size
    ext = np.concatenate([data, data[:7]]).astype(np.uint64)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(7):
        key = (key << np.uint64(8)) | ext[j:j + n]
    key.sort()
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    sizes = np.diff(np.concatenate([starts, [n]]))
    sizes = sizes[sizes > 1]
    return list(zip((np.cumsum(sizes) - sizes).tolist(), sizes.tolist()))


@pytest.mark.parametrize("which", ["shallow", "deep", "tiny"])
def test_planted_inputs_put_the_groups_where_they_say(which):
    """no GPU: the construction above really puts groups of the listed sizes on the slots just before, on and just behind
    multiples of the window's nominal range, and round 2 takes the tile sorter that the fillers are meant to choose: A
    (unresolved suffixes) and ngroups as the host reads them behind round 1 of the cyclic form"""
    data, targets = _PLANTED[which]()
    assert data.size <= 1000000
    groups = _groups_after_round1(data)
    have = set(groups)
    for start, size in targets:
        assert (start, size) in have, (start, size)
    assert {(s % WIN if s % WIN < WIN // 2 else s % WIN - WIN) for s, _ in targets} == {-1, 0, 1}
    assert sorted({size for _, size in targets}) == sorted({s for s, _ in (_DEEP if which == "deep" else _SHALLOW)})
    A, ngroups = sum(size for _, size in groups), len(groups)
    assert A >= 2 * 4096                                        # the tile sorters take the round (tile_sorted_round in bwt_rules.h)
    assert (A // ngroups < 5) == (which == "tiny"), (A, ngroups)      # radix_tile_sorter: counting / bitonic below 5, LDS radix from 5 on


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
@pytest.mark.parametrize("which", ["shallow", "deep", "tiny"])
def test_groups_on_window_borders(hip, oracle, which, cyclic):
    """shallow, deep: round 2 through bwt_tile_sort_radix; tiny: through bwt_tile_sort, whose window prologue is the same code"""
    data, _ = _PLANTED[which]()
    _check_bwt(hip, oracle, data, data.size, cyclic)


# ---- equal rank keys inside a group ----------------------------------------------------------------------------------------
def _pages(page_len, copies, seed):
    """a page repeated `copies` times, each copy followed by one byte of its own: the suffixes at one page offset form a group
    whose members carry EQUAL rank keys round after round (the next difference is up to page_len bytes away), so they must stay
    one group with one new head; 40 copies take the counting path of the tile sorter, 70 and 300 the bitonic / radix paths"""
    page = recipes.textgen(page_len, seed)
    return np.concatenate([np.concatenate([page, np.array([48 + i % 200], dtype=np.uint8)]) for i in range(copies)])


EQUAL_KEY_INPUTS = {
    "pages_40x5000": lambda: _pages(5000, 40, 21),
    "pages_70x5000": lambda: _pages(5000, 70, 22),
    "pages_300x1500": lambda: _pages(1500, 300, 23),
}


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
@pytest.mark.parametrize("name", sorted(EQUAL_KEY_INPUTS))
def test_equal_rank_keys_stay_one_group(hip, oracle, name, cyclic):
    data = EQUAL_KEY_INPUTS[name]()
    _check_bwt(hip, oracle, data, data.size, cyclic)


# ---- groups of more than 1024 suffixes in rounds > 2, and the whole-array fallbacks -------------------------------------------
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


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
@pytest.mark.parametrize("name", sorted(FALLBACK_INPUTS))
def test_large_groups_and_fallbacks(hip, oracle, name, cyclic):
    data, block_len = FALLBACK_INPUTS[name]()
    _check_bwt(hip, oracle, data, block_len, cyclic)


# ---- unsegmented round 1 in front of the new rounds >= 2 ------------------------------------------------------------------
# The inputs as expressions: the child process that sorts and the test that asks the oracle build the same bytes from them.
# "long_scan": 1,000,000 + 34 * 3,000 = 1,102,000 bytes in blocks of 99,981 = 12 blocks (the last 2,209 bytes).  Unsegmented,
# round 1 sorts them as ONE segment of M = 1,102,000 keys = ceil(M / 4096) = 270 tiles, more than the 256 up to which the radix
# passes scan a segment's tile counts in one workgroup: the passes take the three-kernel scan (rs_scan_chunk_sum / _mid /
# _apply), which no segmented sort reaches (a block has at most 2^20 - 2 suffixes = 256 tiles).
_UNSEG_INPUTS = {
    "mixed": "np.concatenate([recipes.textgen(250000, 51), np.tile(recipes.textgen(3000, 52), 40), recipes.textgen(30000, 53)])",
    "long_scan": "np.concatenate([recipes.textgen(1000000, 61), np.tile(recipes.textgen(3000, 62), 34)])",
}


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic,which", [(True, "mixed"), (False, "mixed"), (True, "long_scan"), (False, "long_scan")],
                         ids=["cyclic", "sentinel", "cyclic-long_scan", "sentinel-long_scan"])
def test_unsegmented_round1_multi_block(oracle, cyclic, which):
    """CJS_NO_SEGMENTED_SORT=1 (read per call; set for a child process so that no other test sees it): round 1 sorts all blocks
    as one array with the block id on top of the key, rounds >= 2 are the same kernels"""
    block_len = 99981
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes, numpy as np; "
            "d = %s; "
            "rc, U, pidx = support.HipLib().stage_bwt(d, %d, %s); "
            "print(rc, support.sha256(U), ','.join(str(int(p)) for p in pidx))" % (_UNSEG_INPUTS[which], block_len, cyclic))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, CJS_NO_SEGMENTED_SORT="1"),
                         cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    rc_s, sha, pidx_s = out.stdout.split()
    data = eval(_UNSEG_INPUTS[which], {"np": np, "recipes": recipes})
    if which == "long_scan":
        assert data.size == 1102000 and -(-data.size // block_len) == 12 and -(-data.size // 4096) == 270
    want_u, want_p = [], []
    for k in range(-(-data.size // block_len)):
        eu, ep = (oracle.bwt_cyclic if cyclic else oracle.bwt_sentinel)(data[k * block_len:(k + 1) * block_len])
        want_u.append(eu); want_p.append(int(ep))
    assert rc_s == "0"
    assert pidx_s == ",".join(str(p) for p in want_p)
    assert sha == support.sha256(np.concatenate(want_u))
