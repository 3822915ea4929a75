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
from bwt_cases import DEEP as _DEEP, EQUAL_KEY_INPUTS, FALLBACK_INPUTS, PLANTED as _PLANTED, SHALLOW as _SHALLOW, WIN, groups_after_round1

ROOT = support.ROOT


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


# ---- planted groups at chosen places of the compacted array: the construction is bwt_cases.planted -------------------------
@pytest.mark.parametrize("which", ["shallow", "deep", "tiny"])
def test_planted_inputs_put_the_groups_where_they_say(which):
    """no GPU: the construction (bwt_cases.planted) really puts groups of the listed sizes on the slots just before, on and just behind
    multiples of the window's nominal range, and round 2 takes the tile sorter that the fillers are meant to choose: A
    (unresolved suffixes) and ngroups as the host reads them behind round 1 of the cyclic form"""
    data, targets = _PLANTED[which]()
    assert data.size <= 1000000
    groups = groups_after_round1([data], 7)
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


# ---- equal rank keys inside a group (bwt_cases.pages) ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
@pytest.mark.parametrize("name", sorted(EQUAL_KEY_INPUTS))
def test_equal_rank_keys_stay_one_group(hip, oracle, name, cyclic):
    data = EQUAL_KEY_INPUTS[name]()
    _check_bwt(hip, oracle, data, data.size, cyclic)


# ---- groups of more than 1024 suffixes in rounds > 2, and the whole-array fallbacks (bwt_cases.FALLBACK_INPUTS) -----------------
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
