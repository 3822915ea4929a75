"""The suffix sort over blocks of different lengths (bwt_run_var, the geometry of the batched compressor) against the oracle, block
by block, through cjs_stage_bwt_var.

That geometry is an instantiation of its own of every templated kernel of the sort (bwt_init_keys, both tile sorters,
bwt_gather_keys, the forms of bwt_apply, bwt_flush_active, bwt_pidx) with rules that the fixed geometry never uses: the slots
behind a block's end are holes that round 1 must resolve as singletons; round 1 is always unsegmented and its depth follows
the number of blocks, because the block id and the hole bit share the key with the symbols (7 symbols up to 128 blocks, 6 up to
32768, 5 beyond: depths 5 and 6 exist only here, and the later rounds then run at h = 5, 10, 20, .. or 6, 12, 24, ..); every
cyclic wrap takes the block's own length; and the "only equal rotations are left" exit compares h with the stride, so a short
periodic block beside a long one stays an unsplit group for many rounds.

Every GPU case compares each block's BWT bytes and primary index with oracle.bwt_cyclic of that block, exactly.  The tests
without the gpu mark show on the CPU, with a model of round 1 (bwt_cases.groups_after_round1), that the inputs put their groups
where the cases say, and pin the block counts at which the depth changes."""
import numpy as np
import pytest

import recipes
from bwt_cases import (DEEP, EQUAL_KEY_INPUTS, FALLBACK_INPUTS, PLANTED, SHALLOW, WIN, groups_after_round1, round1_depth_var)

TS_MAXGRP = 1024     # bwt_rules.h: the tile sorters take groups up to this size, larger ones make the deferral trip
MAX_SLOTS = 9000000  # nb * stride of the largest call: 46 bytes of workspace per slot (BwtWork::bytes_needed) stay below 0.5 GB


def _stride(blocks):
    return (max(b.size for b in blocks) + 15) & ~15


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


_oracle_memo = {}    # block bytes -> (U, pidx): the calls of one case that share blocks ask the oracle once


def _want(oracle, blk, memo):
    if not memo:
        return oracle.bwt_cyclic(blk)
    key = blk.tobytes()
    if key not in _oracle_memo:
        _oracle_memo[key] = oracle.bwt_cyclic(blk)
    return _oracle_memo[key]


def _check_var(hip, oracle, blocks, stride=None, hole_fill=0, memo=False):
    """one call of cjs_stage_bwt_var, every block against the oracle; returns [(U_k, pidx_k)]"""
    blocks = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
    stride = stride or _stride(blocks)
    assert len(blocks) * stride <= MAX_SLOTS
    rc, U, pidx = hip.stage_bwt_var(blocks, stride, hole_fill)
    assert rc == 0, "cjs_stage_bwt_var: %d (%d blocks, stride %d)" % (rc, len(blocks), stride)
    for k, blk in enumerate(blocks):
        eu, ep = _want(oracle, blk, memo)
        assert pidx[k] == ep, "pidx block %d: got %d want %d (n=%d, %d blocks, stride %d, fill %#x)" % (k, pidx[k], ep, blk.size, len(blocks), stride, hole_fill)
        if not np.array_equal(U[k], eu):
            bad = np.nonzero(U[k] != eu)[0]
            raise AssertionError("BWT bytes differ in block %d at %d positions, first %d (n=%d, %d blocks, stride %d, fill %#x)"
                                 % (k, bad.size, bad[0], blk.size, len(blocks), stride, hole_fill))
    return [(U[k].copy(), int(pidx[k])) for k in range(len(blocks))]


def _stats(blocks, d):
    groups = groups_after_round1(blocks, d)
    return groups, sum(size for _, size in groups), len(groups)


# ---- the depth of round 1 ---------------------------------------------------------------------------------------------------
def test_round1_depth_thresholds():
    """the block counts the depth cases below rely on (tests/host/bwt_rules_check.cc holds the same four against the header)"""
    assert [round1_depth_var(nb) for nb in (1, 2, 128, 129, 32768, 32769, 33000, 65535)] == [7, 7, 7, 6, 6, 5, 5, 5]


# ---- a. groups on the borders of the tile sorters' windows, depth 7 -------------------------------------------------------------
# The planted inputs of test_gpu_bwt_flags.py as one of three blocks.  The compacted array is in block order, so as block 0 the
# planted groups keep their slots and the groups of the two text blocks follow them.  "front": a block of 3072 bytes stands in
# front, a random string of 1536 bytes twice over: cyclically every rotation has an equal twin, so all its 3072 suffixes are
# unresolved behind round 1 (and stay so until h >= stride: groups of equal rotations) and the planted groups move by exactly one
# window.  The tiny fillers of "tiny" keep round 2 in the counting / bitonic sorter although text brings larger groups.
def _front_block():
    half = np.random.default_rng(104).integers(0x40, 0x80, WIN // 2, dtype=np.uint8)
    return np.concatenate([half, half])


def _border_case(which, front):
    """(blocks, [(start slot, size)] of the planted groups in the compacted array of the whole call)"""
    data, targets = PLANTED[which]()
    text = [recipes.textgen(data.size // 2, 71), recipes.textgen(data.size // 10, 72)]
    if not front:
        return [data] + text, targets
    return [_front_block(), data] + text[1:], [(s + WIN, m) for s, m in targets]


_BORDER_CASES = [(w, f) for w in ("shallow", "deep", "tiny") for f in (False, True)]
_BORDER_IDS = ["%s%s" % (w, "-front" if f else "") for w, f in _BORDER_CASES]


@pytest.mark.parametrize("which,front", _BORDER_CASES, ids=_BORDER_IDS)
def test_border_cases_put_the_groups_where_they_say(which, front):
    blocks, targets = _border_case(which, front)
    assert len(blocks) == 3 and round1_depth_var(len(blocks)) == 7 and len(blocks) * _stride(blocks) <= MAX_SLOTS
    groups, A, ngroups = _stats(blocks, 7)
    have = set(groups)
    for start, size in targets:
        assert (start, size) in have, (start, size)
    assert {(s % WIN if s % WIN < WIN // 2 else s % WIN - WIN) for s, _ in targets} == {-1, 0, 1}
    assert sorted({size for _, size in targets}) == sorted({s for s, _ in (DEEP if which == "deep" else SHALLOW)})
    assert A >= 2 * 4096                                        # the tile sorters take the round (tile_sorted_round in bwt_rules.h)
    assert (A // ngroups < 5) == (which == "tiny"), (A, ngroups)      # radix_tile_sorter: counting / bitonic below 5, LDS radix from 5 on
    if front:      # the block in front holds slots [0, WIN) of the compacted array, all of them
        assert sum(size for start, size in groups if start < WIN) == WIN and min(start for start, _ in groups if start >= WIN) == WIN


@pytest.mark.gpu
@pytest.mark.parametrize("which,front", _BORDER_CASES, ids=_BORDER_IDS)
def test_groups_on_window_borders(hip, oracle, which, front):
    blocks, _ = _border_case(which, front)
    _check_var(hip, oracle, blocks)


# ---- b. equal rank keys inside a group ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EQUAL_KEY_INPUTS))
def test_equal_rank_keys_stay_one_group(hip, oracle, name):
    data = EQUAL_KEY_INPUTS[name]()
    _check_var(hip, oracle, [data, recipes.textgen(data.size // 2, 73), recipes.textgen(data.size // 10, 74)])


# ---- c. large groups and the fallbacks ----------------------------------------------------------------------------------------
def _large_group_case(name):
    if name in ("text_plus_period12", "text_plus_period7"):      # the longest of two blocks, text beside it in the tile sorters
        data, n = FALLBACK_INPUTS[name]()
        return [data[:n], recipes.textgen(300000, 75)]
    if name == "period2_900k":
        # ONE block: two groups of 450,000 suffixes, so D = 900,000 deferred suffixes exceed half of the workspace's cap = nb *
        # stride slots (deferred_overflow) and bwt_gather_keys<VarGeom> runs in front of the whole-array sort.  With two or more
        # blocks this branch cannot be reached: D <= the longest block <= stride <= cap / 2.
        return [FALLBACK_INPUTS[name]()[0]]
    if name == "repeats_3_blocks":      # the three small repeat inputs in one call
        return [FALLBACK_INPUTS[k]()[0] for k in ("repeats_5k", "repeats_7k", "repeats_9k")]
    assert name == "tiny_batch_40"      # the everyday batch of tiny inputs: 40 blocks of 1..300 bytes
    lens = np.random.default_rng(6).integers(1, 301, 40)
    lens[:2] = (1, 300)
    return [recipes.textgen(int(n), 300 + k) for k, n in enumerate(lens)]


_LARGE_GROUP_CASES = ["text_plus_period12", "text_plus_period7", "period2_900k", "repeats_3_blocks", "tiny_batch_40"]


@pytest.mark.parametrize("name", _LARGE_GROUP_CASES)
def test_large_group_cases_are_what_they_say(name):
    blocks = _large_group_case(name)
    groups, A, ngroups = _stats(blocks, round1_depth_var(len(blocks)))
    largest = max(size for _, size in groups)
    cap = len(blocks) * _stride(blocks)
    deferred = sum(size for _, size in groups if size > TS_MAXGRP)
    if name.startswith("text_plus"):      # deferral trip beside tile-sorted groups: a large group, room to sort it apart
        assert len(blocks) == 2 and blocks[0].size > blocks[1].size
        assert A >= 2 * 4096 and largest > TS_MAXGRP and 0 < deferred <= cap // 2 and A - deferred >= 2 * 4096, (A, largest, deferred)
    elif name == "period2_900k":          # over half of the workspace deferred
        assert len(blocks) == 1 and A >= 2 * 4096 and deferred > cap // 2, (A, deferred, cap)
    elif name == "repeats_3_blocks":      # each block alone is near or below the 8192 suffixes of the whole-array path; together
        # they give round 2 to the tile sorters, and the blocks' repeats end at different depths, so A falls below 8192 on the way
        assert len(blocks) == 3 and [b.size for b in blocks] == [5000, 7000, 9000]
        alone = [_stats([b], 7)[1] for b in blocks]
        assert A == sum(alone) and 2 * 4096 <= A and min(alone) < 2 * 4096 and largest <= TS_MAXGRP, (A, alone, largest)
    else:                                 # whole-array from round 2 on
        assert len(blocks) == 40 and min(b.size for b in blocks) == 1 and max(b.size for b in blocks) == 300
        assert 0 < A < 2 * 4096, A


@pytest.mark.gpu
@pytest.mark.parametrize("name", _LARGE_GROUP_CASES)
def test_large_groups_and_fallbacks(hip, oracle, name):
    _check_var(hip, oracle, _large_group_case(name))


# ---- d. lengths and holes ------------------------------------------------------------------------------------------------------
_D_STRIDE = 20000
_SHORT_LENGTHS = (1, 2, 3, 5, 6, 7, 8)      # at or below the depth of round 1 (and one past it): the key wraps, several times


def _short_blocks():
    return [np.full(n, 0x61, np.uint8) for n in _SHORT_LENGTHS] + [np.arange(0x41, 0x41 + n, dtype=np.uint8) for n in _SHORT_LENGTHS]


def _length_blocks():
    """the blocks of case d by name, in no particular order"""
    b = {"equal_%d" % n: blk for n, blk in zip(_SHORT_LENGTHS, _short_blocks()[:len(_SHORT_LENGTHS)])}
    b.update({"distinct_%d" % n: blk for n, blk in zip(_SHORT_LENGTHS, _short_blocks()[len(_SHORT_LENGTHS):])})
    b["ab_x50"] = np.tile(_u8(b"ab"), 50)
    b["abc_x33"] = np.tile(_u8(b"abc"), 33)
    b["aaa"] = _u8(b"aaa")
    b["abcab_cut_at_97"] = np.tile(_u8(b"abcab"), 20)[:97].copy()      # a period that does not divide the length
    b["ab_x2000"] = np.tile(_u8(b"ab"), 2000)                          # periodic and long enough for two groups above TS_MAXGRP
    b["text_stride"] = recipes.textgen(_D_STRIDE, 76)                  # the long block: the periodic ones wait for h >= stride
    b["text_stride_minus_1"] = recipes.textgen(_D_STRIDE - 1, 77)
    b["text_stride_minus_15"] = recipes.textgen(_D_STRIDE - 15, 78)
    b["text_7000"] = recipes.textgen(7000, 79)
    # leading bytes at or above 0x80 in front of holes: the hole bit sits right above the first symbol of the round-1 key
    b["high_bytes_300"] = np.random.default_rng(9).integers(0x80, 0x100, 300, dtype=np.uint8)
    b["ff_x5"] = np.full(5, 0xFF, np.uint8)
    b["ab_x50_again"] = b["ab_x50"].copy()                             # exact repeats at other slots
    b["text_7000_again"] = b["text_7000"].copy()
    return b


def test_length_blocks_are_what_they_say():
    b = _length_blocks()
    blocks = list(b.values())
    assert round1_depth_var(len(blocks)) == 7 and _stride(blocks) == _D_STRIDE
    assert {_D_STRIDE, _D_STRIDE - 1, _D_STRIDE - 15} <= {x.size for x in blocks}
    # the periodic blocks are all equal rotations: none of their suffixes is ever resolved, at any depth below the stride
    for name in ("equal_2", "equal_8", "ab_x50", "abc_x33", "aaa", "ab_x2000"):
        assert _stats([b[name]], 7)[1] == b[name].size, name
    assert 97 % 5 != 0 and _stats([b["abcab_cut_at_97"]], 7)[1] < 97      # the cut breaks the period: not all rotations equal
    for n in _SHORT_LENGTHS:
        assert _stats([b["distinct_%d" % n]], 7)[1] == 0                  # distinct bytes: round 1 resolves the block, wrapped key or not


@pytest.mark.gpu
def test_lengths_and_holes(hip, oracle):
    """four calls over the same blocks: holes filled with 0x00 and 0xFF, blocks by descending length (the order of the batch
    compressor) and shuffled; every call against the oracle, and every block the same in all four and at both its slots"""
    b = _length_blocks()
    names = sorted(b)
    by_len = sorted(names, key=lambda k: -b[k].size)
    shuffled = [names[i] for i in np.random.default_rng(7).permutation(len(names))]
    assert by_len != shuffled
    runs = {}
    for order_name, order in (("descending", by_len), ("shuffled", shuffled)):
        for fill in (0x00, 0xFF):
            try:
                res = _check_var(hip, oracle, [b[k] for k in order], _D_STRIDE, fill, memo=True)
            except AssertionError as e:
                raise AssertionError("%s order: %s (blocks: %s)" % (order_name, e, order))
            runs[(order_name, fill)] = dict(zip(order, res))
    first = runs[("descending", 0x00)]
    for key, got in runs.items():
        for k in names:
            assert got[k][1] == first[k][1] and np.array_equal(got[k][0], first[k][0]), "block %s differs between %s and descending / 0x00" % (k, key)
        for k in ("ab_x50", "text_7000"):
            assert got[k][1] == got[k + "_again"][1] and np.array_equal(got[k][0], got[k + "_again"][0]), (k, key)
    # equal rotations: the primary index is the last row of the group of rotation 0 (the rows of rotation 0's class end there)
    assert first["aaa"][1] == 2 and first["ab_x50"][1] == 49 and first["equal_8"][1] == 7


# ---- e. round 1 at depth 6 -----------------------------------------------------------------------------------------------------
_E_STRIDE = 32768


def _depth6_blocks():
    """129 blocks in slots of 32768; without the last one the same call runs at depth 7"""
    rng = np.random.default_rng(8)
    blocks = [np.tile(recipes.textgen(1500, 23), 20)[:_E_STRIDE].copy(),      # 30,000 bytes, all unresolved behind a depth-6 round
              recipes.build({"kind": "concat", "parts": [      # a period-12 stretch inside text: 12 groups of 1250 suffixes
                  {"kind": "textgen", "n": 10000, "seed": 81}, {"kind": "repeat", "unit_hex": "6162636465666768696a6b6c", "n": 15000},
                  {"kind": "textgen", "n": 5000, "seed": 82}]}),
              recipes.textgen(_E_STRIDE, 83), recipes.textgen(_E_STRIDE - 1, 84)]
    blocks += _short_blocks()
    blocks += [np.tile(_u8(b"ab"), 50), np.tile(_u8(b"abc"), 33), _u8(b"aaa")]
    k = 0
    while len(blocks) < 129:
        n = int(rng.integers(1, _E_STRIDE + 1))
        blocks.append(recipes.textgen(n, 400 + k) if k % 3 == 0 else (rng.integers(0, 2 if k % 3 == 1 else 4, n) + 0x30).astype(np.uint8))
        k += 1
    return blocks


def test_depth6_blocks_are_what_they_say():
    blocks = _depth6_blocks()
    assert len(blocks) == 129 and _stride(blocks) == _E_STRIDE and len(blocks) * _E_STRIDE <= MAX_SLOTS
    assert round1_depth_var(len(blocks)) == 6 and round1_depth_var(len(blocks) - 1) == 7
    groups0, A0, ng0 = _stats(blocks[:1], 6)
    assert (A0, ng0, max(size for _, size in groups0)) == (30000, 1248, 280)
    assert max(size for _, size in _stats(blocks[1:2], 6)[0]) > TS_MAXGRP
    for d, bl in ((6, blocks), (7, blocks[:-1])):
        groups, A, ngroups = _stats(bl, d)
        assert A >= 2 * 4096 and max(size for _, size in groups) > TS_MAXGRP and ngroups > 1000, (d, A, ngroups)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [129, 128], ids=["129_blocks_depth6", "128_blocks_depth7"])
def test_round1_depth6_and_its_neighbour(hip, oracle, nb):
    _check_var(hip, oracle, _depth6_blocks()[:nb], _E_STRIDE, memo=True)


# ---- f. round 1 at depth 5 -----------------------------------------------------------------------------------------------------
_F_STRIDE = 256
# nb, symbols of the alphabet -> round-1 depth; suffixes per group behind round 1 at or above 5 (LDS radix tile sorter) or below
_DEPTH5_CASES = {"33000_blocks_2sym": (33000, 2, 5, True), "33000_blocks_4sym": (33000, 4, 5, False), "32768_blocks_2sym": (32768, 2, 6, False)}


def _depth5_blocks(nb, alphabet):
    rng = np.random.default_rng(1)
    lens = rng.integers(1, _F_STRIDE + 1, nb)
    return [(rng.integers(0, alphabet, int(n)) + 48).astype(np.uint8) for n in lens]


@pytest.mark.parametrize("name", sorted(_DEPTH5_CASES))
def test_depth5_blocks_are_what_they_say(name):
    nb, alphabet, depth, radix = _DEPTH5_CASES[name]
    blocks = _depth5_blocks(nb, alphabet)
    assert len(blocks) == nb and nb * _F_STRIDE <= MAX_SLOTS and _stride(blocks) == _F_STRIDE and min(b.size for b in blocks) == 1
    assert round1_depth_var(nb) == depth
    groups, A, ngroups = _stats(blocks, depth)
    assert A >= 2 * 4096 and (A // ngroups >= 5) == radix, (A, ngroups)
    if name == "33000_blocks_2sym":
        assert (A, ngroups) == (4088548, 793901)
        assert _stats(blocks, 7)[1] > A // 2       # (a lower bound for depth 10, the next round: over half are still unresolved)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_DEPTH5_CASES))
def test_round1_depth5_and_its_neighbour(hip, oracle, name):
    nb, alphabet, _, _ = _DEPTH5_CASES[name]
    _check_var(hip, oracle, _depth5_blocks(nb, alphabet), _F_STRIDE)


# ---- the entry point's argument checks ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stage_refuses_what_the_kernels_cannot_take(hip):
    ok = [_u8(b"banana"), _u8(b"ab")]
    for blocks, stride in ((ok, 0), (ok, 8), (ok, 24), ([_u8(b"banana"), _u8(b"")], 16), ([np.zeros(17, np.uint8)], 16), ([], 16),
                           ([_u8(b"a")] * 65536, 16)):
        rc, U, pidx = hip.stage_bwt_var(blocks, stride)
        assert rc == -32 and U is None, (len(blocks), stride, rc)      # CJS_E_INVALID_ARG
    rc, U, pidx = hip.stage_bwt_var(ok, 16)
    assert rc == 0 and bytes(U[0]) == b"nnbaaa" and pidx[0] == 3 and bytes(U[1]) == b"ba" and pidx[1] == 0
