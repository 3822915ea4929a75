"""Packed cyclic round 1 with 4-byte records in its last phase-1 passes (radix.hip: radix_passes_pk1; bwt_round1.hip:
bwt_phase2_records): inputs aimed at what that form added.

The last passes of phase 1 carry byte 2 | position only, so bwt_phase2_records takes the 40-bit class key (bytes 2..6) of every
slot back from the block text: three aligned words around the suffix, a byte-wise wrapping path for the positions whose eight
bytes cross the block end, and the same for the slot in front of a tile and for the probes of the class search.  The records
carry no block parity any more, so classes are kept apart at block starts by slot number alone.  Every case compares bytes and
primary index block by block with the oracle's cyclic BWT through cjs_stage_bwt, as tests/test_gpu_bwt_flags.py does.
"""
import numpy as np
import pytest

import recipes

TILE = 4096          # RS_TILE: slots per workgroup of the radix passes and of the record rebuild
LOOKBACK = 64        # slots in front of a tile that wave 0 looks at before it searches (class_head_before_by)


def _check_bwt(hip, oracle, data, block_len):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    rc, U, pidx = hip.stage_bwt(data, block_len, True)
    assert rc == 0
    nb = -(-data.size // block_len)
    for k in range(nb):
        blk = data[k * block_len:(k + 1) * block_len]
        eu, ep = oracle.bwt_cyclic(blk)
        got = U[k * block_len:k * block_len + blk.size]
        assert pidx[k] == ep, "pidx block %d: got %d want %d (n=%d)" % (k, pidx[k], ep, blk.size)
        if not np.array_equal(got, eu):
            bad = np.nonzero(got != eu)[0]
            raise AssertionError("BWT bytes differ in block %d at %d positions, first %d (n=%d)" % (k, bad.size, bad[0], blk.size))


def _random_bytes(n, seed):
    """all 256 byte values, those >= 0x80 included"""
    return np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8)


def _text_with_high_bytes(n, seed):
    """textgen with every seventh byte or so moved into the upper half"""
    t = recipes.textgen(n, seed).copy()
    t[np.random.RandomState(seed + 1000).rand(n) < 0.15] |= 0x80
    return t


# ---- the inputs of the class search ----------------------------------------------------------------------------------------
PLANT = np.array([0x60, 0xC1, 0x85, 0xF0, 0x99], dtype=np.uint8)
PLANT_COPIES, PLANT_IN_FRONT = 70, 67


def _equal_bytes():
    return np.full(3 * TILE + 5, 0xE1, dtype=np.uint8)


def _abcde():
    return np.resize(np.frombuffer(b"abcde", dtype=np.uint8), 12293).copy()


def _planted_5gram():
    """9,001 random bytes above 0x60 but for exactly TILE - PLANT_IN_FRONT bytes below it, and PLANT 70 times: 0x60 only opens
    a copy of PLANT, so the suffixes with PLANT at bytes 2..6 are one class of 70, the bytes in front of each copy are random,
    and what sorts in front of the class are the suffixes with a low byte at byte 2: the class takes slots 4029..4098, 67 of
    them in front of the second tile"""
    rs = np.random.RandomState(77)
    n = 9001
    t = rs.randint(0x61, 256, size=n).astype(np.uint8)
    starts = 100 + 120 * np.arange(PLANT_COPIES)
    free = np.ones(n, dtype=bool)
    for s in starts:
        t[s:s + 5] = PLANT
        free[s:s + 5] = False
    low = rs.permutation(np.flatnonzero(free))[:TILE - PLANT_IN_FRONT]
    t[low] = rs.randint(0, 0x60, size=low.size).astype(np.uint8)
    return t


CLASS_SEARCH = {"equal_bytes": _equal_bytes, "abcde": _abcde, "planted_5gram": _planted_5gram}


def classes_after_phase1(block):
    """(first slot, size) of the classes of bytes 2..6 of one cyclic block in sorted order, singletons included: what phase 1
    of the packed round 1 leaves and bwt_phase2_records looks for (bwt_cases.groups_after_round1 with five bytes from byte 2
    on, on the array as it stands and not compacted)"""
    n = block.size
    b = block.astype(np.uint64)
    i = np.arange(n)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(2, 7):
        key = (key << np.uint64(8)) | b[(i + j) % n]
    key.sort()
    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    return list(zip(starts.tolist(), np.diff(np.concatenate([starts, [n]])).tolist()))


def _runs_into_tile(classes):
    """(first slot, size, members in front of the tile start) of the classes that cross the start of a tile"""
    out = []
    for s, size in classes:
        edge = -(-s // TILE) * TILE
        if s < edge < s + size:
            out.append((s, size, edge - s))
    return out


def test_class_search_inputs_do_what_their_names_say():
    """no GPU: the three inputs really make the look-back of 64 slots fail at a tile start, each in its own way"""
    c = classes_after_phase1(_equal_bytes())
    assert c == [(0, 3 * TILE + 5)]                                    # one class over three tiles and five slots: every search runs back to slot 0
    c = classes_after_phase1(_abcde())
    assert sorted(size for _, size in c) == [1, 1, 1, 1, 2457, 2458, 2458, 2458, 2458]      # classes of about 2,458; the singles reach around the end
    into = _runs_into_tile(c)
    assert len(into) == 3 and all(front > LOOKBACK for _, _, front in into)
    assert any(s > 0 for s, _, _ in into)                              # a search that ends inside the block, not at its first slot
    data = _planted_5gram()
    assert data.size == 9001 and int((data == PLANT[0]).sum()) == PLANT_COPIES
    c = classes_after_phase1(data)
    big = [(s, size) for s, size in c if size > LOOKBACK]
    assert big == [(TILE - PLANT_IN_FRONT, PLANT_COPIES)]              # the one class of more than 64 members
    assert _runs_into_tile(c)[0] == (TILE - PLANT_IN_FRONT, PLANT_COPIES, PLANT_IN_FRONT) and PLANT_IN_FRONT > LOOKBACK
    plants = np.flatnonzero(data == PLANT[0])
    assert len({(int(data[p - 2]), int(data[p - 1])) for p in plants}) > LOOKBACK      # otherwise distinct: bytes 0..1 of those suffixes differ


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLASS_SEARCH))
def test_class_search(hip, oracle, name):
    data = CLASS_SEARCH[name]()
    _check_bwt(hip, oracle, data, data.size)


# ---- wrap paths of the gather --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097])
def test_one_block_of_every_wrap_length(hip, oracle, n):
    """positions 0 and n - 6 .. n - 1 take the byte-wise path; below 7 bytes every position does and wraps more than once"""
    _check_bwt(hip, oracle, _random_bytes(n, 500 + n), n)


@pytest.mark.gpu
def test_wrap_keys_meet_plain_keys(hip, oracle):
    """the last six bytes repeat the first six: suffixes that reach their key around the block end share classes with suffixes
    that read it straight"""
    data = _random_bytes(5003, 41)
    data[-6:] = data[:6]
    _check_bwt(hip, oracle, data, data.size)


# ---- block geometry: odd strides, the two-sweep regroup (>= 8 blocks) --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tail", [5, 0], ids=["9x4099+5", "8x4099"])
def test_odd_strides(hip, oracle, tail):
    nb = 9 if tail else 8
    _check_bwt(hip, oracle, _text_with_high_bytes(nb * 4099 + tail, 31 + tail), 4099)


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [8, 2])
def test_identical_neighbours(hip, oracle, copies):
    """equal blocks side by side: without a parity bit in the records a class must still end at the block start"""
    _check_bwt(hip, oracle, np.tile(_text_with_high_bytes(4099, 57), copies), 4099)
