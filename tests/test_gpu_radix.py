"""The radix sorter on its own (csrc/radix.hip through cjs_stage_radix) against the stable sort of radix_cases.reference: both key
widths, with and without values and the byte-per-key array, plain and in segments, every form of the tile scan, keys made from the
block text, stale workspaces and the two refusals.  Every comparison is exact, every call leaves its guards alone.

What runs: rs_hist<K, GEN> (uint64 / uint32 plain, uint64 GEN), rs_hist_bytes (DIG), rs_scan_bins, the three-kernel chunk scan
(above 256 tiles a segment), rs_scatter<K, GEN, NOVAL> for both K (GEN for uint64).  Out of reach here and held elsewhere:
radix_passes_pk1 and the packed cyclic key source (test_gpu_bwt_round1_narrow.py)."""
import numpy as np
import pytest

import radix_cases as rc

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 1024 + 17          # four tiles, the last one short (one whole wave and 17 keys)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8193, N)
RANGES64 = ((0, 8), (0, 32), (0, 64), (48, 64), (8, 24), (4, 20), (0, 13), (32, 45), (52, 62))
RANGES32 = ((0, 8), (0, 32), (8, 24), (4, 20), (0, 13), (20, 30))          # (52, 62) and (20, 30): the last digit clipped at the key width
ONES = {4: np.uint32(0xFFFFFFFF), 8: np.uint64(0xFFFFFFFFFFFFFFFF)}


@pytest.fixture(scope="module")
def L():
    import torch
    assert torch.cuda.is_available()
    return rc.bind()


def rand_keys(rng, n, key_bytes):
    """random bits everywhere: below lo_bit, above hi_bit and between hi_bit and the end of the last digit as well"""
    lo32 = rng.randint(0, 2 ** 32, n, dtype=np.uint64)
    return lo32.astype(np.uint32) if key_bytes == 4 else (rng.randint(0, 2 ** 32, n, dtype=np.uint64) << np.uint64(32)) | lo32


def with_field(rng, field, lo, key_bytes, width=16):
    """keys that carry `field` in bits [lo, lo + width) and random bits elsewhere"""
    keys = rand_keys(rng, field.size, key_bytes).astype(np.uint64)
    keys = (keys & ~np.uint64(((1 << width) - 1) << lo)) | (field.astype(np.uint64) << np.uint64(lo))
    return keys.astype(rc.key_dtype(key_bytes))


def agree(L, keys, vals, geom, lo, hi, what, **kw):
    """one call against the reference: exact keys and values, guards whole -> the result"""
    res = rc.run(L, keys, vals, geom, lo, hi, **kw)
    assert res.rc == 0, (what, res.rc)
    assert res.guard_bad == 0, (what, "guard bytes written", res.guard_bad)
    passes = -(-(hi - lo) // 8)
    assert res.cur == passes % 2, (what, res.cur)
    want_k, want_v = rc.reference(keys, vals, geom, lo, hi)
    try:
        rc.check(res.keys, None if vals is None else res.vals, want_k, want_v, geom)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    if vals is None:
        assert (res.vals.view(np.uint8) == rc.CANARY).all(), (what, "values written by a key-only call")
    return res


# ---------------------------------------------------------------- plain sorts
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "n%d" % n)
def test_plain_sizes(L, n):
    rng = np.random.RandomState(n)
    idx = np.arange(n, dtype=np.uint32)          # the input index as the value: a pass that is not stable shows
    for key_bytes, ranges in ((8, RANGES64), (4, RANGES32)):
        for lo, hi in ranges:
            keys = rand_keys(rng, n, key_bytes)
            if hi - lo <= 16:          # few values in bits [lo, hi), so that equal sort words meet in every wave; nothing above hi is touched
                thin = 0xF0F0 & ((1 << (hi - lo)) - 1)
                keys &= rc.key_dtype(key_bytes)(~(thin << lo) & int(ONES[key_bytes]))
            if (hi - lo) % 8 and n >= 63:          # the bits between hi and the end of the last digit are random: a sort on [lo, hi) alone gives another order
                narrow = (keys.astype(np.uint64) >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)
                word = rc.sort_word(keys, key_bytes, lo, hi)
                assert (word != narrow).any(), (key_bytes, lo, hi)
                assert not np.array_equal(np.argsort(word, kind="stable"), np.argsort(narrow, kind="stable")), (key_bytes, lo, hi)
            for vals in (idx, None):
                agree(L, keys, vals, rc.plain(n), lo, hi, "%d-byte keys, %s, bits (%d, %d)" % (key_bytes, "key-only" if vals is None else "values", lo, hi))


def _contents():
    rng = np.random.RandomState(1234)
    i = np.arange(N)
    r16 = rng.randint(0, 2 ** 16, N)
    grp = i // 64          # the 64 keys that the lanes of a wave rank in one step
    out = {
        "all keys equal": np.full(N, 0x1234),
        "already sorted": np.sort(r16),
        "reversed": np.sort(r16)[::-1].copy(),
        "two values alternating": np.where(i & 1, 0xFEFD, 0x0102),
        "one digit on a fifth of the keys": np.where(rng.rand(N) < 0.2, (r16 & 0xFF00) | 0x20, r16),
        "every wave's 64 lanes on one digit": ((grp * 37) & 0xFF) | (((grp * 101 + 7) & 0xFF) << 8),
        "256 digits once each, then one digit for the rest": np.where(i < 256, i | ((255 - i) << 8), 0x0707),
    }
    return {k: v.astype(np.uint64) for k, v in out.items()}


CONTENTS = _contents()
FORMS = ((8, 0), (8, 40), (4, 8))          # (key bytes, lo_bit) of the 16-bit field the contents go into


def content_keys(name, key_bytes, lo):
    rng = np.random.RandomState(len(name) + lo)
    if name == "all keys ~0 with distinct values":
        return np.full(N, ONES[key_bytes])
    if name == "~0 keys only in the short last tile":
        keys = with_field(rng, rng.randint(0, 2 ** 16 - 1, N), lo, key_bytes)          # no real key has the field all ones
        keys[3 * 4096:] = ONES[key_bytes]
        return keys
    return with_field(rng, CONTENTS[name], lo, key_bytes)


ALL_CONTENTS = sorted(CONTENTS) + ["all keys ~0 with distinct values", "~0 keys only in the short last tile"]


@pytest.mark.parametrize("name", ALL_CONTENTS)
def test_contents(L, name):
    idx = np.arange(N, dtype=np.uint32)
    for key_bytes, lo in FORMS:
        keys = content_keys(name, key_bytes, lo)
        agree(L, keys, idx, rc.plain(N), lo, lo + 16, "%s, %d-byte keys from bit %d" % (name, key_bytes, lo))
        agree(L, keys, None, rc.plain(N), lo, lo + 16, "%s, %d-byte keys from bit %d, key-only with the byte array" % (name, key_bytes, lo), flags=rc.DIG)
        # (no product caller moves values beside the byte array, but radix_passes and the entry admit it: rs_scatter<K, false, false> leaving digits)
        agree(L, keys, idx, rc.plain(N), lo, lo + 16, "%s, %d-byte keys from bit %d, values with the byte array" % (name, key_bytes, lo), flags=rc.DIG)


@pytest.mark.parametrize("name", ("one digit on a fifth of the keys", "every wave's 64 lanes on one digit", "~0 keys only in the short last tile"))
def test_stale_workspace(L, name):
    """the product reuses its workspaces: whatever the counts, totals, chunk sums, byte array and buffers held, the result is the same"""
    idx = np.arange(N, dtype=np.uint32)
    for key_bytes, lo in FORMS:
        keys = content_keys(name, key_bytes, lo)
        got = []
        for fill in (0x00, 0xFF, 0xA5):
            res = agree(L, keys, idx, rc.plain(N), lo, lo + 16, "%s, workspace filled with %#x" % (name, fill), work_fill=fill)
            got.append((res.keys.tobytes(), res.vals.tobytes()))
            agree(L, keys, None, rc.plain(N), lo, lo + 16, "%s, key-only with the byte array, workspace filled with %#x" % (name, fill), work_fill=fill, flags=rc.DIG)
        assert got[0] == got[1] == got[2]


# ---------------------------------------------------------------- the tile scan: one workgroup up to 256 tiles a segment, three kernels in chunks of 64 tiles above
def skewed(rng, n, nbytes):
    """digits whose counts differ from tile to tile: the lowest byte is drawn below a bound that moves with the tile, the others lean low"""
    tile = np.arange(n) // rc.TILE
    keys = (rng.rand(n) * (1 + (tile * 37) % 256)).astype(np.uint64)
    for b in range(1, nbytes):
        keys |= (rng.rand(n) ** 2 * 256).astype(np.uint64) << np.uint64(8 * b)
    return keys


@pytest.mark.parametrize("form", ("k64_values_0_16", "k32_alone_0_32"))
@pytest.mark.parametrize("short", (0, 5), ids=("whole", "short"))
@pytest.mark.parametrize("tps", (256, 257, 320, 321), ids=lambda t: "tiles%d" % t)
def test_tile_scan_forms(L, tps, short, form):
    n = tps * rc.TILE - short
    rng = np.random.RandomState(tps + short)
    if form == "k64_values_0_16":
        k64 = skewed(rng, n, 2) | (rand_keys(rng, n, 8) << np.uint64(16))
        agree(L, k64, np.arange(n, dtype=np.uint32), rc.plain(n), 0, 16, "64-bit keys with values on (0, 16), %d keys" % n)
    else:
        k32 = skewed(rng, n, 4).astype(np.uint32)
        agree(L, k32, None, rc.plain(n), 0, 32, "32-bit keys alone on (0, 32), %d keys" % n)


# ---------------------------------------------------------------- segments
SEGS = ((2, 4096, 4096), (2, 4097, 1), (3, 5001, 5000), (3, 8195, 4097), (5, 8195, 4096), (7, 100, 100), (7, 100, 1), (2, 12289, 1))
FULL_SEGS = tuple(g for g in SEGS if g[1] == g[2]) + ((2, 4097, 4097), (3, 5001, 5001), (3, 8195, 8195), (2, 12289, 12289))
seg_id = lambda g: "%dx%d_last%d" % tuple(g)


def seg_keys(rng, geom, key_bytes):
    """the same multiset of keys in every segment (the last one: a part of it), each in an order of its own: a record that strays into
    another segment changes that segment.  values = the index in the whole array"""
    geom = rc.Geom(*geom)
    base = rand_keys(rng, geom.stride, key_bytes)
    base[rng.rand(geom.stride) < 0.3] = base[0]          # and many equal keys in each
    keys = np.concatenate([base[rng.permutation(geom.stride)][: b - a] for a, b in rc.seg_bounds(geom)])
    return geom, keys, np.arange(keys.size, dtype=np.uint32)


@pytest.mark.parametrize("g", SEGS, ids=seg_id)
def test_segments_64(L, g):
    rng = np.random.RandomState(sum(g))
    geom, keys, vals = seg_keys(rng, g, 8)
    cap = rc.cap_for(geom)
    agree(L, keys, vals, geom, 0, 24, "64-bit keys with values on (0, 24)", work_cap=cap)
    # the shape of the last two passes of the packed round 1 (bwt_round1.hip): key-only, the second pass counts from the byte array,
    # whose segments start at every byte alignment with the odd strides
    agree(L, keys, None, geom, 48, 64, "64-bit keys alone with the byte array on (48, 64)", work_cap=cap, flags=rc.DIG)
    agree(L, keys, vals, geom, 3, 22, "64-bit keys with values and the byte array on (3, 22): three digits, the last ends inside", work_cap=cap, flags=rc.DIG)


@pytest.mark.parametrize("g", FULL_SEGS, ids=seg_id)
def test_segments_32_through_radix_pass_segments(L, g):
    rng = np.random.RandomState(sum(g) + 1)
    geom, keys, vals = seg_keys(rng, g, 4)
    cap = rc.cap_for(geom)
    agree(L, keys, vals, geom, 0, 16, "32-bit keys with values on (0, 16)", work_cap=cap, flags=rc.SEGMENTS)
    agree(L, keys, None, geom, 8, 24, "32-bit keys alone on (8, 24)", work_cap=cap, flags=rc.SEGMENTS)
    # the inverse BWT's one pass (dec_ibwt.hip): keys (i << 8) | byte, the slots behind a block's bytes hold 0xFF, the counts of the
    # digit come with the call
    keys = np.zeros(rc.n_of(geom), dtype=np.uint32)
    counts = [max(1, geom.stride - 1 - 37 * s) for s in range(geom.nseg)]
    for count, (a, b) in zip(counts, rc.seg_bounds(geom)):
        by = rng.choice(np.array([0, 1, 97, 98, 254, 255], dtype=np.uint32), count)
        by[-1] = 0xFF          # a real 0xFF next to the padding
        keys[a: a + count] = (np.arange(count, dtype=np.uint32) << np.uint32(8)) | by
        keys[a + count: b] = 0xFF
    hist = rc.first_hist(keys, geom, 0)
    res = agree(L, keys, None, geom, 0, 8, "the inverse BWT's pass with its counts handed in", work_cap=cap, flags=rc.SEGMENTS | rc.FIRST_HIST, hist=hist)
    for count, (a, b) in zip(counts, rc.seg_bounds(geom)):          # (what the decoder relies on: the padding behind everything real)
        assert count < b - a and (res.keys[a + count: b] == 0xFF).all() and res.keys[a + count - 1] == (((count - 1) << 8) | 0xFF)


def test_refusals_leave_everything_alone(L):
    rng = np.random.RandomState(77)
    # more tiles than the workspace has rows: 400 segments of one tile each, hist_tiles_for(6400) = 260.  BOTH conditions of the
    # refusal hold here (segs_for(6400) = 2 as well): a workspace carved by hist_tiles_for / segs_for has 256 more rows than it
    # has segments' totals, and a geometry of n <= cap keys has at most ceil(cap / 4096) + nseg tiles, so the tile condition
    # cannot be met alone through this entry; the segment condition alone is the case below
    geom, keys, vals = seg_keys(rng, (400, 16, 16), 8)
    res = rc.run(L, keys, vals, geom, 0, 8, work_cap=rc.n_of(geom))
    assert res.rc == rc.E_INVALID and res.guard_bad == 0 and rc.untouched(res)
    # more segments than the workspace has totals for: segs_for(n < 65536) = 2
    for g, flags, key_bytes in (((3, 5001, 5000), 0, 8), ((3, 5001, 5001), rc.SEGMENTS, 4)):
        geom, keys, vals = seg_keys(rng, g, key_bytes)
        assert rc.n_of(geom) < 65536
        res = rc.run(L, keys, vals, geom, 0, 8, work_cap=rc.n_of(geom), flags=flags)
        assert res.rc == rc.E_INVALID and res.guard_bad == 0 and rc.untouched(res)
        hist = rc.first_hist(keys, geom, 0)
        res = rc.run(L, keys, vals, geom, 0, 8, work_cap=rc.n_of(geom), flags=flags | rc.FIRST_HIST, hist=hist)
        assert res.rc == rc.E_INVALID and res.guard_bad == 0 and rc.untouched(res)
        agree(L, keys, vals, geom, 0, 8, "the same with room", work_cap=rc.cap_for(geom), flags=flags | rc.FIRST_HIST, hist=hist)


def test_argument_errors(L):
    keys, vals = np.arange(300, dtype=np.uint64), np.arange(300, dtype=np.uint32)
    k32 = keys.astype(np.uint32)
    text = np.zeros(300, dtype=np.uint8)
    bad = (dict(geom=rc.plain(300), lo=16, hi=8), dict(geom=rc.plain(300), lo=8, hi=8), dict(geom=rc.plain(300), lo=-8, hi=8), dict(geom=rc.plain(300), lo=0, hi=65),
           dict(geom=rc.Geom(4, 100, 0), lo=0, hi=8), dict(geom=rc.Geom(1, 400, 300), lo=0, hi=8), dict(geom=rc.Geom(3, 100, 100), lo=0, hi=8, work_cap=299),
           dict(geom=rc.plain(300), lo=0, hi=8, work_cap=(1 << 26) + 1), dict(geom=rc.plain(300), lo=0, hi=8, flags=16),
           dict(geom=rc.Geom(3, 100, 100), lo=0, hi=8, flags=rc.SEGMENTS),                         # 8-byte keys
           dict(geom=rc.plain(300), lo=0, hi=8, flags=rc.FIRST_HIST),                               # no counts
           dict(geom=rc.plain(300), lo=0, hi=63, flags=rc.GEN),                                     # no text
           dict(geom=rc.plain(300), lo=0, hi=64, flags=rc.GEN, text=text), dict(geom=rc.plain(300), lo=0, hi=63, flags=rc.GEN | rc.DIG, text=text))
    for kw in bad:
        res = rc.run(L, keys, vals, **kw)
        assert res.rc == rc.E_INVALID and rc.untouched(res), kw
    for kw in (dict(geom=rc.plain(300), lo=0, hi=33), dict(geom=rc.Geom(3, 100, 100), lo=0, hi=8, flags=rc.SEGMENTS | rc.DIG),
               dict(geom=rc.Geom(4, 90, 30), lo=0, hi=8, flags=rc.SEGMENTS), dict(geom=rc.plain(300), lo=0, hi=32, flags=rc.GEN, text=text)):
        res = rc.run(L, k32, vals, **kw)
        assert res.rc == rc.E_INVALID and rc.untouched(res), kw
    res = rc.run(L, np.zeros(0, np.uint32), None, rc.Geom(1, 0, 0), 0, 8)          # no keys: nothing to do, nothing launched
    assert res.rc == 0 and rc.untouched(res)


# ---------------------------------------------------------------- keys made from the block text (the segmented sentinel sort of round 1)
# odd strides: the segments' bases fall at every byte alignment.  4103 / 4104 / 4105: the first tile of a segment is copied as
# aligned words when 4096 + 8 bytes of the segment lie behind its start, byte by byte otherwise
GENS = ((1, 8209, 8209), (3, 8209, 8209), (3, 8209, 4100), (3, 8209, 1), (4, 12301, 4097), (2, 4103, 4103), (2, 4104, 4104), (2, 4105, 4105))


def gen_text(kind, geom):
    rng = np.random.RandomState(geom.stride + geom.n_last)
    n = rc.n_of(geom)
    if kind == "uniform bytes":          # 0x00 and 0xFF among them: the symbol 256 needs the ninth bit
        text = rng.randint(0, 256, n).astype(np.uint8)
        text[rng.rand(n) < 0.1] = 0xFF
        text[rng.rand(n) < 0.1] = 0x00
        return text
    if kind == "a run to the segment's end":          # of two suffixes inside the run the shorter one sorts first
        text = rng.randint(97, 101, n).astype(np.uint8)
        for a, b in rc.seg_bounds(geom):
            text[max(a, b - 600): b] = 0x61
        return text
    base = rng.randint(97, 99, geom.stride).astype(np.uint8)          # the same text in every segment: only bit 63 and the end tell them apart
    return np.concatenate([base[: b - a] for a, b in rc.seg_bounds(geom)])


@pytest.mark.parametrize("kind", ("uniform bytes", "a run to the segment's end", "the same text in every segment"))
@pytest.mark.parametrize("g", GENS, ids=seg_id)
def test_generated_keys(L, g, kind):
    geom = rc.Geom(*g)
    text = gen_text(kind, geom)
    keys, vals = rc.gen_keys(text, *geom)
    want_k, want_v = rc.reference(keys, vals, geom, 0, 63)
    for fill in (0xA5, 0x00):
        res = rc.run(L, None, None, geom, 0, 63, key_bytes=8, flags=rc.GEN, text=text, work_cap=rc.cap_for(geom), work_fill=fill)
        assert res.rc == 0 and res.guard_bad == 0 and res.cur == 0, (res.rc, res.guard_bad, res.cur)
        rc.check(res.keys, res.vals, want_k, want_v, geom)
