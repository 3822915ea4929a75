"""Suffix sort rounds >= 2 with the group heads as one byte per slot (ghead[], written by bwt_apply, read by both tile sorters and
by bwt_gather_keys): inputs on the edges that this form moves.

Between a regroup and the next sort the grouping travels as one head byte per surviving slot, no longer as a 32-bit group ordinal.
The window prologue of the tile sorters (ts_window in bwt_tile_sort.hip) takes its head masks straight from those bytes and looks
back over the 1024 head bytes in front of the window for the start of the group that runs into it; the keys that the sorters leave
for the deferral kernels carry the head bit where the ordinal was, and bwt_defer_count / bwt_defer_gather number the deferred
groups from it; bwt_gather_keys (the whole-array fallbacks) counts the ordinals out of the head bytes.  Every GPU case compares
each block's BWT bytes and primary index with the oracle's, exactly, through the stage entry points cjs_stage_bwt and
cjs_stage_bwt_var.  The tests without the gpu mark show with the CPU model of round 1 (bwt_cases.groups_after_round1) that the
inputs put their groups where the cases say.

The planted inputs are built like bwt_cases.planted, from an explicit list of group sizes in array order: a unit (3 id bytes that
sort in front of everything else, in id order, then random bytes) occurs m times, each occurrence followed by random bytes of
its own, so after round 1 (depth 7) the array that round 2 sorts STARTS with groups of exactly the listed sizes.  The byte
behind a unit (and the byte in front of the next one) differs between its first 192 occurrences and the two bytes there between
all, so the suffixes one byte into a unit and one byte in front of it add groups only for m > 192, m slots each, and those two
bytes off none (they sort behind all planted groups)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import recipes
import support
from bwt_cases import groups_after_round1

ROOT = support.ROOT
TS_WIN, TS_MAXGRP, TS_NOM = 4096, 1024, 3072      # bwt_rules.h


def _phrases(plan, unit_len, sep_len, seed):
    """plan: group sizes (>= 2) in array order -> bytes"""
    rng = np.random.default_rng(seed)
    assert len(plan) < 64 * 128 * 128 and min(plan) >= 2
    parts, done = [], 0
    for uid, m in enumerate(plan):
        unit = rng.integers(0x40, 0x80, unit_len, dtype=np.uint8)
        unit[0] = uid >> 14; unit[1] = 0x80 | ((uid >> 7) & 127); unit[2] = 0x80 | (uid & 127)
        occ = rng.integers(0x40, 0x80, (m, unit_len + sep_len), dtype=np.uint8)
        occ[:, :unit_len] = unit
        i = np.arange(m)
        occ[:, unit_len] = 0x40 + rng.permutation(192)[i % 192]; occ[:, unit_len + 1] = 0x40 + (i // 192) % 64
        j = done + i                 # (numbered over all occurrences: what follows is an occurrence of any unit)
        occ[:, -1] = 0x40 + j % 192; occ[:, -2] = 0x40 + (j // 192) % 64
        done += m
        parts.append(occ)
    occs = np.concatenate(parts)
    return np.ascontiguousarray(occs[rng.permutation(occs.shape[0])].reshape(-1))      # no unit is periodic in the text


def _plan(targets, filler, total):
    """targets: [(start slot, size)] ascending; fillers of `filler` (2: 2, 3, 2, 3, ..) between them and up to `total` slots"""
    plan, at = [], 0

    def fill(gap):
        nonlocal at
        assert gap == 0 or gap >= 2, gap
        while gap >= 2 * filler + 2:
            m = filler + (len(plan) & 1 if filler == 2 else 0)
            plan.append(m); gap -= m; at += m
        if gap > 3 and filler == 2:
            plan.append(2); gap -= 2; at += 2
        if gap:
            plan.append(gap); at += gap

    for start, size in targets:
        fill(start - at)
        assert at == start
        plan.append(size); at += size
    fill(total - at)
    return plan


# ---- groups that straddle a window edge -------------------------------------------------------------------------------------
# A group starts d slots in front of slot TS_NOM and another d slots in front of slot 2 * TS_NOM, and both run on into the next
# window: windows 1 and 2 find their start by the look-back over the head bytes (d = 1: the last byte of the look-back; 63, 64:
# either side of a mask word and of a wave's share of the look-back; 1023: its first byte but one; 1024 members from there reach
# one slot into the window, the largest group that has an owner).  d = 0: slots TS_NOM and 2 * TS_NOM are heads themselves and the
# group in front ends on the edge.  The array that round 2 sorts has between 2 * TS_WIN and 3 * TS_WIN + 7 slots, so the tile
# sorters take it, the last window short.  Fillers of 2 and 3 put round 2 through the counting sorter, fillers
# of 8 through the LDS radix sorter.
_STRADDLE = [(d, f) for d in (1, 63, 64, 1023, 0) for f in (2, 8)]
_STRADDLE_IDS = ["%s-%s" % ("head_on_edge" if d == 0 else "%d_in_front" % d, "counting" if f == 2 else "radix") for d, f in _STRADDLE]


def _straddle_targets(d):
    size = min(d + 40, TS_MAXGRP) if d else 50
    return [(TS_NOM - d, size), (2 * TS_NOM - d, size)]


def _straddle_input(d, filler):
    total = 3 * TS_NOM + 7 if d != 1023 else 2 * TS_NOM + 1024      # (the two groups of 1024 bring 4096 more slots along: see _phrases)
    return _phrases(_plan(_straddle_targets(d), filler, total), 7, 5, 200 + d + filler)


@pytest.mark.parametrize("d,filler", _STRADDLE, ids=_STRADDLE_IDS)
def test_straddle_inputs_put_the_groups_where_they_say(d, filler):
    groups = groups_after_round1([_straddle_input(d, filler)], 7)
    have = set(groups)
    for start, size in _straddle_targets(d):
        assert (start, size) in have, (start, size)
        assert start + size > (start + d) and (start + d) % TS_NOM == 0      # the group reaches into the window behind the edge
    A, ngroups = sum(size for _, size in groups), len(groups)
    assert 2 * TS_WIN <= A <= 3 * TS_WIN + 7, A
    assert (A // ngroups >= 5) == (filler == 8), (A, ngroups)            # radix_tile_sorter in bwt_rules.h


def _check_bwt(hip, oracle, data, block_len, cyclic):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    rc, U, pidx = hip.stage_bwt(data, block_len, cyclic)
    assert rc == 0
    for k in range(-(-data.size // block_len)):
        blk = data[k * block_len:(k + 1) * block_len]
        eu, ep = (oracle.bwt_cyclic if cyclic else oracle.bwt_sentinel)(blk)
        got = U[k * block_len:k * block_len + blk.size]
        assert pidx[k] == ep, "pidx block %d: got %d want %d (n=%d cyclic=%s)" % (k, pidx[k], ep, blk.size, cyclic)
        if not np.array_equal(got, eu):
            bad = np.nonzero(got != eu)[0]
            raise AssertionError("BWT bytes differ in block %d at %d positions, first %d (n=%d cyclic=%s)" % (k, bad.size, bad[0], blk.size, cyclic))


@pytest.mark.gpu
@pytest.mark.parametrize("d,filler", _STRADDLE, ids=_STRADDLE_IDS)
def test_groups_straddling_a_window_edge(hip, oracle, d, filler):
    data = _straddle_input(d, filler)
    _check_bwt(hip, oracle, data, data.size, True)


# ---- the own / defer boundary ---------------------------------------------------------------------------------------------------
# Groups of 1023, 1024 (owned) and 1025 members (deferred: its slots get head bit | rank key as keys), then two deferred groups
# back to back (only the head bit tells them apart: bwt_defer_count numbers them 1 and 2) and one deferred group across two
# window edges.  Units of 15 bytes: the groups pass round 2 whole and split in round 3, so both rounds defer.
_BOUNDARY = [(TS_NOM - 700, 1023), (2 * TS_NOM - 700, 1024), (3 * TS_NOM - 700, 1025), (4 * TS_NOM + 100, 1025), (4 * TS_NOM + 1125, 1300),
             (6 * TS_NOM - 1500, 3500)]


def _boundary_input(filler):
    return _phrases(_plan(_BOUNDARY, filler, 8 * TS_NOM), 15, 4, 300 + filler)


@pytest.mark.parametrize("filler", [2, 8], ids=["counting", "radix"])
def test_boundary_input_puts_the_groups_where_it_says(filler):
    groups = groups_after_round1([_boundary_input(filler)], 7)
    have = set(groups)
    for t in _BOUNDARY:
        assert t in have, t
    assert _BOUNDARY[3][0] + _BOUNDARY[3][1] == _BOUNDARY[4][0]
    deferred = sum(size for _, size in groups if size > TS_MAXGRP)
    assert 0 < deferred <= _boundary_input(filler).size // 2 and sum(size for _, size in groups) >= 2 * TS_WIN


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
@pytest.mark.parametrize("filler", [2, 8], ids=["counting", "radix"])
def test_groups_of_1023_1024_1025(hip, oracle, filler, cyclic):
    """(sentinel: the BWTC form, which keeps a suffix array and takes rank key 0 past the end)"""
    data = _boundary_input(filler)
    _check_bwt(hip, oracle, data, data.size, cyclic)


# ---- the whole-array fallbacks: group ordinals counted out of the head bytes ---------------------------------------------------
def _overflow_input():
    """one long run plus text: more than half of the workspace's slots are deferred, the whole array is sorted by keys that
    bwt_gather_keys makes over many tiles (per-tile head counts, scanned)"""
    return np.concatenate([recipes.textgen(9000, 91), np.zeros(30000, np.uint8), recipes.textgen(11000, 92)])


def _small_round_input():
    """two blocks with fewer than 8192 unresolved suffixes behind round 1, in two tiles: bwt_gather_keys counts the heads in
    front of its tile by itself"""
    return np.tile(recipes.textgen(900, 42), 8)[:7000].copy(), 3500


def test_fallback_inputs_are_what_they_say():
    data = _overflow_input()
    groups = groups_after_round1([data], 7)
    assert sum(size for _, size in groups if size > TS_MAXGRP) > data.size // 2 and sum(size for _, size in groups) >= 2 * TS_WIN
    data, n = _small_round_input()
    groups = groups_after_round1([data[:n], data[n:]], 7)
    A = sum(size for _, size in groups)
    assert data.size == 2 * n and 4096 < A < 2 * TS_WIN and len(groups) > 2, A


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
def test_more_than_half_deferred(hip, oracle, cyclic):
    data = _overflow_input()
    _check_bwt(hip, oracle, data, data.size, cyclic)


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
def test_two_blocks_below_the_tile_sorters(hip, oracle, cyclic):
    data, n = _small_round_input()
    _check_bwt(hip, oracle, data, n, cyclic)


# ---- one batch of blocks of different lengths (bwt_run_var) --------------------------------------------------------------------
@pytest.mark.gpu
def test_blocks_of_different_lengths(hip, oracle):
    """the straddling groups, the own / defer boundary, a long run and small repeats as blocks of one call: the kernels'
    VarGeom instantiations, the sorted positions of a window spanning several blocks"""
    blocks = [_straddle_input(64, 2), _boundary_input(8), _overflow_input(), _small_round_input()[0], recipes.textgen(20000, 93),
              np.tile(np.frombuffer(b"ab", np.uint8), 50)]
    stride = (max(b.size for b in blocks) + 15) & ~15
    rc, U, pidx = hip.stage_bwt_var(blocks, stride, 0)
    assert rc == 0
    for k, blk in enumerate(blocks):
        eu, ep = oracle.bwt_cyclic(blk)
        assert pidx[k] == ep, "pidx block %d: got %d want %d" % (k, pidx[k], ep)
        assert np.array_equal(U[k], eu), "BWT bytes differ in block %d" % k


# ---- both tile sorters on the text of the benchmark ----------------------------------------------------------------------------
# Three blocks of 20,000 bytes of the benchmark's text (tools/textgen.c, seed 1).  Blocks that short never reach the five suffixes
# per group from which round 2 takes the LDS radix sorter (the CPU model of round 1: 20,340 unresolved suffixes in 6,120 groups,
# 3.3 per group; other seeds 3.3 .. 3.8; the 900,000-byte blocks of the benchmark 7.7), so the input comes in two forms: "plain",
# three consecutive stretches of 20,000 bytes, which the counting sorter takes in every tile-sorted round; and "copies", every block
# 4,000 bytes of that text five times over, which the radix sorter takes (in the sentinel form for four rounds, then the counting
# sorter).  Which sorter a round took is read from the round lines
# that CJS_DEBUG prints (read once per process: a child process): radix_tile_sorter(A, ngroups) of the counts in front of it.
_BENCH_TEXT = {
    "plain": "recipes.textgen(60000, 1)",
    "copies": "np.concatenate([np.tile(recipes.textgen(60000, 1)[k * 20000:k * 20000 + 4000], 5) for k in range(3)])",
}
_ROUND = re.compile(r"\[cjs bwt\] round (\d+) h=(\d+) A=(\d+) bits=(\d+) -> A'=(\d+) groups=(\d+)")


@pytest.mark.gpu
@pytest.mark.parametrize("cyclic", [True, False], ids=["cyclic", "sentinel"])
@pytest.mark.parametrize("which", sorted(_BENCH_TEXT))
def test_bench_text_through_both_tile_sorters(oracle, which, cyclic):
    block_len = 20000
    code = ("import sys; sys.path.insert(0, 'tests'); import torch, support, recipes, numpy as np; "
            "rc, U, pidx = support.HipLib().stage_bwt(%s, %d, %s); "
            "print(rc, support.sha256(U), ','.join(str(int(p)) for p in pidx))" % (_BENCH_TEXT[which], block_len, cyclic))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, CJS_DEBUG="1"), cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-1500:]
    rc_s, sha, pidx_s = out.stdout.split()
    data = eval(_BENCH_TEXT[which], {"np": np, "recipes": recipes})
    assert data.size == 3 * block_len
    want_u, want_p = [], []
    for k in range(3):
        eu, ep = (oracle.bwt_cyclic if cyclic else oracle.bwt_sentinel)(data[k * block_len:(k + 1) * block_len])
        want_u.append(eu); want_p.append(int(ep))
    assert rc_s == "0" and pidx_s == ",".join(str(p) for p in want_p) and sha == support.sha256(np.concatenate(want_u))
    rounds = [tuple(int(x) for x in m.groups()) for m in _ROUND.finditer(out.stderr)]
    assert len(rounds) >= 3 and [r[0] for r in rounds] == list(range(1, len(rounds) + 1)), out.stderr[-1500:]
    sorters = []
    for prev, cur in zip(rounds, rounds[1:]):          # the sort of round cur[0] ran over prev's survivors and groups
        A, ngroups = prev[4], prev[5]
        assert cur[2] == A
        if A >= 2 * TS_WIN:
            sorters.append("radix" if ngroups and A // ngroups >= 5 else "counting")
    # (sentinel copies: groups of five that lose a member per round to the block's end, 5.8 .. 5.0 suffixes per group for four rounds,
    # then below 5 -- both sorters in one call)
    want = {"counting"} if which == "plain" else {"radix"} if cyclic else {"radix", "counting"}
    assert len(sorters) >= 2 and set(sorters) == want, rounds
