"""The crafted-block streams of bzblocks.py on the CPU: every case decodes in the oracle to what the Python restatement of the
reference's loops (bzblocks.walk / bzblocks.expand) says, and the geometry the GPU tests (test_gpu_dec_backend.py) count on --
which bytes are count bytes at which border, how much a tile expands to, how long the walks between splitters are, where the
start slot lies, how long the cycle through it is -- is measured here, not assumed."""
import collections

import numpy as np
import pytest

import bzblocks as bz


def _walked(oracle, case):
    """(tt, orig, w, slots, start) of a one-block case"""
    made = case.make()
    if made[0] == "tt":
        tt, orig = made[1], made[2]
    else:
        assert len(made[1]) == 1
        tt, orig = oracle.bwt_cyclic(made[1][0])
    w, slots, start = bz.walk(tt, orig)
    if made[0] == "blocks":
        assert np.array_equal(w, made[1][0]), case.name       # the walk visits the bytes the case chose
    return tt, orig, w, slots, start


def _runs(w):
    """(start, length) of the maximal stretches of equal bytes"""
    w = np.asarray(w)
    edges = np.concatenate([[0], np.nonzero(w[1:] != w[:-1])[0] + 1, [w.size]])
    return edges[:-1], np.diff(edges)


@pytest.mark.parametrize("name", [c.name for c in bz.CASES])
def test_case_decodes_in_oracle(oracle, name):
    stream, want = bz.stream(oracle, bz.BY_NAME[name])
    rc, got = oracle.bzip2_decompress(stream)
    assert rc == 0, (name, rc)
    assert got.tobytes() == want, (name, bz.first_difference(got, want))


def test_families_are_complete():
    count = collections.Counter(c.family for c in bz.CASES)
    assert count == {"R1": 196, "R2": 180, "R3": 88, "R4": 16, "R5": 7, "R6": 17, "R7": 24, "W1": 11, "W2": 6, "W3": 19, "W4": 43}, count


def test_background_has_no_runs():
    for phase in (0, 2, 3, 5, 11):
        w = bz.lit(40000, phase)
        assert bool((w[1:] != w[:-1]).all()) and int(w.max()) <= 250


def test_r1_count_byte_stands_where_the_name_says():
    for B in bz.R1_BORDERS:
        for d in bz.R1_SHIFTS:
            for case in [bz.BY_NAME["R1-B%d-d%+d-count%d" % (B, d, c)] for c in bz.R1_COUNTS] + \
                        [bz.BY_NAME["R1-B%d-d%+d-run7x11" % (B, d)], bz.BY_NAME["R1-B%d-d%+d-run255x259" % (B, d)]]:
                w = case.make()[1][0]
                at = B + d
                starts, lengths = _runs(w[:at])
                assert starts[-1] == at - 4 and lengths[-1] == 4, case.name          # a run of exactly four ends at B + d - 1
                assert lengths[:-1].max() == 1, case.name
                out = bz.expand(w)
                assert len(out) == case.claims["out_len"], case.name
                assert out[at - 4: at + int(w[at])] == bytes([w[at - 1]]) * (4 + int(w[at])), case.name      # w[B + d] was the count
    assert bz.BY_NAME["R1-B16-d+0-run7x11"].make()[1][0][12:17].tolist() == [7] * 5                         # count byte == run byte


def test_r2_stretches_start_at_every_offset_and_tiles_start_on_count_bytes():
    for v in (0, 1, 4, 5, 255):
        for n in (16383, 16384, 16385, 16388, 32769, 50000):
            assert bz.BY_NAME["R2-v%d-n%d" % (v, n)].make()[1][0].tolist() == [v] * n
            for lead in range(5):
                w = bz.BY_NAME["R2-v%d-n%d-lead%d" % (v, n, lead)].make()[1][0]
                starts, lengths = _runs(w)
                k = int(np.argmax(lengths))
                assert lengths[k] == n and starts[k] % 5 == lead and np.sort(lengths)[-2] == 1
    # in a stretch from the block's start the first byte of every following tile is a count byte (16384 % 5 == 4)
    n = len(bz.expand(np.full(bz.TILE, 255, dtype=np.uint8)))
    assert len(bz.expand(np.full(bz.TILE + 1, 255, dtype=np.uint8))) == n + 255
    assert len(bz.expand(np.full(2 * bz.TILE + 1, 255, dtype=np.uint8))) - len(bz.expand(np.full(2 * bz.TILE, 255, dtype=np.uint8))) == 1


def test_r3_stretches_straddle_the_tile_border():
    seen = set()
    for L in range(4, 15):
        for before in range(1, L):
            w = bz.BY_NAME["R3-len%d-before%d" % (L, before)].make()[1][0]
            starts, lengths = _runs(w)
            k = int(np.argmax(lengths))
            assert lengths[k] == L and starts[k] == bz.TILE - before and w[starts[k]] == 2 and np.sort(lengths)[-2] == 1
            seen.add((L % 5, before % 5))
    assert len(seen) == 25


def test_r5_tiles_expand_to_the_sizes_around_the_staging_limit():
    for case in bz.R_CASES:
        if "tile_out" in case.claims:
            w = case.make()[1][0]
            lo = case.claims["tile"] * bz.TILE
            # (the loop's state after a prefix of w is the state the tile is entered with: the difference is the tile's own output)
            assert len(bz.expand(w[: lo + bz.TILE])) - len(bz.expand(w[:lo])) == case.claims["tile_out"], case.name
            if lo:
                assert w[lo - 4: lo].tolist() == [253] * 4 and w[lo] == 10 and len(bz.expand(w[: lo + 1])) - len(bz.expand(w[:lo])) == 10
    w = bz.BY_NAME["R5-maximal"].make()[1][0]
    assert w.size == bz.TILE + 1 and len(bz.expand(w)) == 848743 and len(bz.expand(w[: bz.TILE])) == 3276 * 259 + 4


def test_r6_every_block_offset_and_output_alignment_occurs():
    blocks = bz.BY_NAME["R6-17-blocks"].make()[1]
    assert [b.size for b in blocks] == [4096 + k for k in range(17)]
    offsets = np.concatenate([[0], np.cumsum([b.size for b in blocks])[:-1]])
    assert sorted(set(int(o) % 16 for o in offsets)) == list(range(16))
    for k in range(16):
        made = bz.BY_NAME["R6-first-block-out%d" % k].make()[1]
        assert made[-1].size == 20000 and len(made) == (2 if k else 1)
        assert sum(len(bz.expand(b)) for b in made[:-1]) == k


def test_r7_count_bytes_collide_with_run_bytes():
    for seed in range(24):
        w = bz.BY_NAME["R7-seed%d" % seed].make()[1][0]
        assert w.size == 40000 + seed and set(np.unique(w).tolist()) == ({0, 1, 2, 3, 254, 255} if seed % 3 == 0 else {0, 1, 2, 3})
        _, lengths = _runs(w)
        assert 2.5 < lengths.mean() < 4.5
        assert int((lengths >= 5).sum()) > 1000                 # stretches of equal bytes above 4: their fifth byte is a count equal to the run's byte
        assert len({int(x) % 5 for x in lengths[lengths >= 4]}) == 5


def test_w1_stretches(oracle):
    every = collections.Counter()
    for case in bz.W_CASES:
        if case.family != "W1":
            continue
        _, _, _, slots, start = _walked(oracle, case)
        assert bz.cycle_length(slots, start) == slots.size, case.name
        got = collections.Counter(bz.stretch_lengths(slots, start))
        assert sum(k * v for k, v in got.items()) == slots.size
        if case.claims["stretches"] is not None:
            assert {k: v for k, v in got.items() if k > 2} == case.claims["stretches"], (case.name, got)
        assert (start % 64 == 0) == case.claims["alias"], (case.name, start)
        every.update(got)
    for length in (383, 384, 385, 767, 768, 769):
        assert every[length] >= 1, length
    assert max(every) >= 20000
    assert bz.stretch_lengths(np.array([5, 64, 7, 8, 128, 9]), 5) == [1, 3, 2]


def test_w2_start_slots(oracle):
    alias, plain = [], []
    for case in bz.W_CASES:
        if case.family in ("W1", "W2"):
            _, _, _, slots, start = _walked(oracle, case)
            assert bz.cycle_length(slots, start) == slots.size, case.name
            if case.family == "W2":
                assert start == case.claims["start"], (case.name, start)
                (alias if start % 64 == 0 else plain).append(slots.size)
    for sizes in (alias, plain):
        assert len(sizes) >= 3 and any(n < 64 for n in sizes) and any(n % 64 == 0 for n in sizes), sizes


def test_w3_cycles(oracle):
    for case in bz.W_CASES:
        if case.family == "W3":
            _, _, _, slots, start = _walked(oracle, case)
            assert bz.cycle_length(slots, start) == case.claims["cycle"], case.name
    assert sorted({c.claims["cycle"] for c in bz.W_CASES if c.family == "W3" and c.claims["cycle"] <= 1000}) == list(bz.W3_PERIODS)


def test_w4_cycles_that_do_not_divide_the_block(oracle):
    odd = 0
    for case in bz.W_CASES:
        if case.family == "W4":
            tt, orig, w, slots, start = _walked(oracle, case)
            cyc = bz.cycle_length(slots, start)
            if "cycle" in case.claims:
                assert cyc == case.claims["cycle"], case.name
            if cyc < tt.size and tt.size % cyc:
                odd += 1
                assert np.array_equal(w, np.resize(w[:cyc], tt.size))
    assert odd >= 4, odd
    names = {c.name for c in bz.W_CASES}
    for n in bz.W4_LENGTHS:
        for alphabet in (3, 256):
            assert "W4-n%d-of%d-orig0" % (n, alphabet) in names and "W4-n%d-of%d-orig%d" % (n, alphabet, n - 1) in names


def test_expand_by_hand():
    assert bz.expand(b"xyzaaaa\x02b") == b"xyzaaaaaab"
    assert bz.expand(b"aaaa") == b"aaaa" and bz.expand(b"aaaa\x00") == b"aaaa" and bz.expand(b"aaaaa") == b"aaaa" + b"a" * 97
    assert bz.expand(b"aaabbbba") == b"aaabbbb" + b"b" * 97                      # the byte decoded by hand starts no run
    assert bz.expand(b"\x05" * 11) == b"\x05" * (4 + 5 + 4 + 5 + 1)
