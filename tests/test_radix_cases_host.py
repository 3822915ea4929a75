"""tests/radix_cases.py without a GPU: the reference against Python's sorted(), the generated keys against a second formulation, and
the checker against results that are wrong on purpose, all made in numpy: the proof that test_gpu_radix.py can fail.  (No broken
kernel is ever run for that.)"""
import numpy as np
import pytest

import radix_cases as rc

N = 3 * 4096 + 1024 + 17


def rand_keys(rng, n, key_bytes):
    return rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(rc.key_dtype(key_bytes)) if key_bytes == 4 else \
        (rng.randint(0, 2 ** 32, n, dtype=np.uint64) << np.uint64(32)) | rng.randint(0, 2 ** 32, n, dtype=np.uint64)


def test_sort_word_is_whole_digits_clipped_at_the_key_width():
    k = np.array([0xFEDCBA9876543210], dtype=np.uint64)
    assert int(rc.sort_word(k, 8, 0, 8)[0]) == 0x10 and int(rc.sort_word(k, 8, 0, 13)[0]) == 0x3210
    assert int(rc.sort_word(k, 8, 4, 20)[0]) == 0x4321 and int(rc.sort_word(k, 8, 32, 45)[0]) == 0xBA98
    assert int(rc.sort_word(k, 8, 0, 64)[0]) == 0xFEDCBA9876543210 and int(rc.sort_word(k, 8, 48, 64)[0]) == 0xFEDC
    assert int(rc.sort_word(k, 8, 52, 62)[0]) == 0xFED                      # two digits from bit 52: clipped at bit 64
    k4 = np.array([0x76543210], dtype=np.uint32)
    assert int(rc.sort_word(k4, 4, 8, 24)[0]) == 0x5432 and int(rc.sort_word(k4, 4, 20, 30)[0]) == 0x765 and int(rc.sort_word(k4, 4, 0, 32)[0]) == 0x76543210


@pytest.mark.parametrize("key_bytes", (4, 8))
def test_reference_against_sorted(key_bytes):
    rng = np.random.RandomState(11 + key_bytes)
    for geom in (rc.plain(1), rc.plain(2), rc.plain(300), rc.Geom(3, 50, 7), rc.Geom(2, 64, 64), rc.Geom(7, 10, 1)):
        n = rc.n_of(geom)
        for lo, hi in ((0, 8), (0, 13), (4, 20), (8, 24), (0, 32)) + (((32, 45), (48, 64), (0, 64)) if key_bytes == 8 else ((20, 30),)):
            keys = rand_keys(rng, n, key_bytes)
            keys[rng.rand(n) < 0.5] &= rc.key_dtype(key_bytes)(0x0F0F0F0F)          # many equal sort words
            vals = rng.permutation(n).astype(np.uint32)
            got_k, got_v = rc.reference(keys, vals, geom, lo, hi)
            width = min(8 * ((hi - lo + 7) // 8), 8 * key_bytes - lo)
            want = []
            for a, b in rc.seg_bounds(geom):
                recs = list(zip(keys[a:b].tolist(), vals[a:b].tolist()))
                want += sorted(recs, key=lambda r: (r[0] >> lo) & ((1 << width) - 1))          # (sorted is stable)
            assert list(zip(got_k.tolist(), got_v.tolist())) == want, (geom, lo, hi)
            only_k, none = rc.reference(keys, None, geom, lo, hi)
            assert none is None and only_k.tolist() == [r[0] for r in want]


def gen_keys_by_columns(text, geom):
    """the second formulation: symbol columns over all positions of a segment at once"""
    text = np.asarray(text, dtype=np.uint8)
    keys = np.zeros(text.size, dtype=np.uint64)
    vals = np.zeros(text.size, dtype=np.uint32)
    for s, (a, b) in enumerate(rc.seg_bounds(geom)):
        sym = np.concatenate([text[a:b].astype(np.uint64) + np.uint64(1), np.zeros(7, np.uint64)])
        k = np.zeros(b - a, dtype=np.uint64)
        for j in range(7):
            k |= sym[j: j + b - a] << np.uint64(9 * (6 - j))
        keys[a:b] = k | (np.uint64(s & 1) << np.uint64(63))
        vals[a:b] = np.arange(b - a)
    return keys, vals


def test_gen_keys_against_the_second_formulation():
    rng = np.random.RandomState(5)
    for geom in (rc.plain(1), rc.plain(6), rc.plain(7), rc.plain(8), rc.Geom(3, 9, 9), rc.Geom(3, 9, 2), rc.Geom(4, 33, 1), rc.Geom(2, 300, 299)):
        n = rc.n_of(geom)
        for text in (rng.randint(0, 256, n), rng.choice([0, 255], n), np.full(n, 0x61), np.zeros(n)):
            got = rc.gen_keys(np.asarray(text, dtype=np.uint8), *geom)
            want = gen_keys_by_columns(text, geom)
            assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), geom
    k, v = rc.gen_keys(np.array([0, 255, 97], dtype=np.uint8), 1, 3, 3)
    assert k.tolist() == [(1 << 54) | (256 << 45) | (98 << 36), (256 << 54) | (98 << 45), 98 << 54] and v.tolist() == [0, 1, 2]
    k, v = rc.gen_keys(np.array([5, 5, 5, 5], dtype=np.uint8), 2, 2, 2)          # the odd segment carries bit 63, and nothing crosses a segment's end
    assert k.tolist() == [(6 << 54) | (6 << 45), 6 << 54, (1 << 63) | (6 << 54) | (6 << 45), (1 << 63) | (6 << 54)] and v.tolist() == [0, 1, 0, 1]


def test_first_hist_rows():
    geom = rc.Geom(2, 5000, 5000)
    keys = (np.arange(10000, dtype=np.uint32) % 5000 << np.uint32(8)) | (np.arange(10000, dtype=np.uint32) % 3)
    h = rc.first_hist(keys, geom, 0)
    assert h.shape == (4, 256) and h.sum(axis=1).tolist() == [4096, 904, 4096, 904] and int(h[:, 3:].sum()) == 0
    assert h[1, :3].tolist() == [int(((np.arange(4096, 5000) % 3) == d).sum()) for d in range(3)]


def test_cap_for_admits_its_geometry():
    for geom in (rc.plain(1), rc.Geom(7, 100, 1), rc.Geom(5, 8195, 4096), rc.Geom(400, 16, 16), rc.Geom(3, 5001, 5000)):
        cap = rc.cap_for(geom)
        assert cap >= rc.n_of(geom) and cap // 65536 + 2 >= geom.nseg and -(-cap // 4096) + cap // 65536 + 258 >= geom.nseg * rc.tiles_per_seg(geom)


def rejects(got_k, got_v, want_k, want_v, geom, slot=None):
    with pytest.raises(AssertionError) as e:
        rc.check(got_k, got_v, want_k, want_v, geom)
    if slot is not None:
        assert rc.where(slot, geom) in str(e.value), str(e.value)
    return str(e.value)


def test_check_accepts_the_reference_and_names_the_place():
    rng = np.random.RandomState(1)
    geom = rc.Geom(3, 8195, 4097)
    keys, vals = rand_keys(rng, rc.n_of(geom), 8), np.arange(rc.n_of(geom), dtype=np.uint32)
    want_k, want_v = rc.reference(keys, vals, geom, 0, 24)
    rc.check(want_k.copy(), want_v.copy(), want_k, want_v, geom)
    rc.check(want_k.copy(), None, want_k, None, geom)
    slot = 8195 + 4096 + 1024 + 65
    assert rc.where(slot, geom) == "slot 13380 = segment 1 + 5185: tile 1, wave 1, lane 1"
    assert rc.where(2 * 8195 + 4096, geom) == "slot 20486 = segment 2 + 4096: tile 1, wave 0, lane 0"
    bad = want_v.copy()
    bad[slot] ^= 1
    msg = rejects(want_k, bad, want_k, want_v, geom, slot)
    assert "1 slots differ" in msg and "value %d" % bad[slot] in msg and "value %d" % want_v[slot] in msg and "key %#x" % want_k[slot] in msg
    rejects(want_k, None, want_k, want_v, geom)                               # values missing
    rejects(want_k[:-1], None, want_k, None, geom)                            # a short array
    rejects(want_k.astype(np.uint32), None, want_k, None, geom)               # another width


def test_check_rejects_an_unstable_permutation_of_equal_keys():
    rng = np.random.RandomState(2)
    geom = rc.plain(N)
    keys = rng.randint(0, 50, N).astype(np.uint64) << np.uint64(8)           # 50 sort words on (8, 16): long runs of equal ones
    vals = np.arange(N, dtype=np.uint32)
    want_k, want_v = rc.reference(keys, vals, geom, 8, 16)
    got_v = want_v.copy()
    i = 2000
    assert want_k[i] == want_k[i + 1]
    got_v[[i, i + 1]] = got_v[[i + 1, i]]                                      # the keys alone cannot tell
    assert np.array_equal(want_k, np.sort(keys))
    rejects(want_k, got_v, want_k, want_v, geom, i)


def test_check_rejects_a_sort_on_the_bits_below_hi_alone():
    rng = np.random.RandomState(3)
    geom = rc.plain(N)
    vals = np.arange(N, dtype=np.uint32)
    for key_bytes, lo, hi in ((8, 0, 13), (8, 32, 45), (8, 4, 17), (4, 8, 21), (4, 0, 13)):
        keys = rand_keys(rng, N, key_bytes)                                   # random bits between hi and the end of the last digit
        want_k, want_v = rc.reference(keys, vals, geom, lo, hi)
        narrow = (keys.astype(np.uint64) >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)
        order = np.argsort(narrow, kind="stable")
        rejects(keys[order], vals[order], want_k, want_v, geom)
        rejects(keys[order], None, want_k, None, geom)


def test_check_rejects_segments_that_mix():
    rng = np.random.RandomState(4)
    geom = rc.Geom(2, 4097, 1)
    base = rand_keys(rng, 4097, 8)
    keys = np.concatenate([base, base[:1]])
    vals = np.arange(4098, dtype=np.uint32)
    want_k, want_v = rc.reference(keys, vals, geom, 0, 24)
    order = np.argsort(rc.sort_word(keys, 8, 0, 24), kind="stable")         # one sort over both segments
    rejects(keys[order], vals[order], want_k, want_v, geom)
    geom = rc.Geom(3, 5001, 5001)                                             # the same multiset in every segment: only the values tell
    base = rand_keys(rng, 5001, 8)
    keys = np.concatenate([base[rng.permutation(5001)] for _ in range(3)])
    vals = np.arange(15003, dtype=np.uint32)
    want_k, want_v = rc.reference(keys, vals, geom, 0, 64)
    got_v = want_v.copy()
    a, b = 10, 5001 + 10
    assert want_k[a] == want_k[b]
    got_v[[a, b]] = got_v[[b, a]]
    rejects(want_k, got_v, want_k, want_v, geom, a)


def test_check_rejects_reordered_all_ones_keys_of_the_short_last_tile():
    rng = np.random.RandomState(6)
    geom = rc.plain(N)
    keys = rand_keys(rng, N, 8) & ~np.uint64(1)
    keys[3 * 4096:] = ~np.uint64(0)                                           # what the kernel pads the short tile with, as real keys
    vals = np.arange(N, dtype=np.uint32)
    want_k, want_v = rc.reference(keys, vals, geom, 0, 16)
    ones = np.nonzero(want_k == ~np.uint64(0))[0]
    assert ones.size == 1024 + 17 and ones[0] == 3 * 4096 and want_v[ones].tolist() == list(range(3 * 4096, N))
    got_v = want_v.copy()
    got_v[ones] = want_v[ones][::-1]
    rejects(want_k, got_v, want_k, want_v, geom, 3 * 4096)
    got_v = want_v.copy()
    got_v[-1] = 0                                                             # the last of them lost to a padding record
    rejects(want_k, got_v, want_k, want_v, geom, N - 1)


def test_check_rejects_one_swapped_pair_at_a_tile_border():
    rng = np.random.RandomState(7)
    geom = rc.plain(N)
    keys, vals = rand_keys(rng, N, 4), np.arange(N, dtype=np.uint32)
    want_k, want_v = rc.reference(keys, vals, geom, 0, 32)
    assert want_k[4095] != want_k[4096]
    got_k, got_v = want_k.copy(), want_v.copy()
    got_k[[4095, 4096]] = got_k[[4096, 4095]]
    got_v[[4095, 4096]] = got_v[[4096, 4095]]
    msg = rejects(got_k, got_v, want_k, want_v, geom, 4095)
    assert "2 slots differ" in msg and "tile 0, wave 3, lane 63" in msg
    rejects(got_k, None, want_k, None, geom, 4095)
