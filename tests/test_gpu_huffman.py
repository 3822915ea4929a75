"""The bzip2 entropy stage (huff.hip) block by block against the oracle, on BOTH implementations of the table refinement:
`huff_block` (one workgroup per block, path 1) and the chain hs_init -> hs_assign / hs_split / hs_count / hs_build ->
hs_finish (many workgroups per block, path 2), through cjs_stage_huff_blocks (tables, then the bare packing of each block).

Every case checks, on both paths: table count, selectors and code lengths = oracle.huff_groups; the block's bit string =
oracle.bzip2_block_bits; the two paths agree.  The inputs aim at the edges of the heuristic (group-count thresholds, exact cost
and usage ties, the length limiter) and at the workgroup boundaries of the kernels (512-group assign steps, 2048 groups per
hs_assign workgroup, 131,072 symbols per hs_count workgroup, 4000-symbol packing tiles).  The last part runs inputs whose
shape takes the chain path inside cjs_bzip2_compress and the batch entry points."""
import heapq

import numpy as np
import pytest

import support

pytestmark = pytest.mark.gpu

PER_BLOCK, CHAIN = 1, 2
GEO = 0.618


def _target(npos):                                  # Bzip2:2150
    return 6 if npos >= 2400 else 5 if npos >= 1200 else 4 if npos >= 600 else 3 if npos >= 200 else 2


def _depth(freq):
    """depth of a plain (unlimited) Huffman tree over all symbols, zero counts included (as StaticHuffman builds it)"""
    h = [(int(f), i, 0) for i, f in enumerate(freq)]
    heapq.heapify(h)
    c = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], c, max(a[2], b[2]) + 1))
        c += 1
    return h[0][2]


def _used(rng, asz, kind):
    """ascending used byte values: a contiguous run, or spread over as many of the 16 coarse groups as asz allows"""
    if kind == "contiguous" or asz == 256:
        s = int(rng.randint(0, 257 - asz))
        return np.arange(s, s + asz, dtype=np.uint8)
    groups = np.unique(np.linspace(0, 15, min(asz, 16)).round().astype(int))
    pick = set(int(g) * 16 + int(rng.randint(16)) for g in groups)
    rest = [b for b in range(256) if b not in pick]
    pick |= set(int(x) for x in rng.choice(rest, asz - len(pick), replace=False))
    u = np.array(sorted(pick), dtype=np.uint8)
    if asz >= 16:
        assert np.unique(u >> 4).size == 16
    return u


def _syms(rng, npos, asz, dist):
    """npos MTF/RLE2 symbols: npos - 1 of 0..asz, then the end-of-block symbol asz + 1"""
    m, k = npos - 1, asz + 1
    if dist == "uniform":
        body = rng.randint(0, k, m)
    elif dist == "dominant":                        # one symbol nearly everywhere: long codes for all the others
        body = np.where(rng.random_sample(m) < 0.995, 0, rng.randint(0, k, m))
    elif dist == "zeros":                           # zero-count symbols inside the alphabet
        body = rng.choice(np.arange(0, k, 3), m)
    elif dist == "geometric":                       # P(s) ~ 0.618^s: Fibonacci-like counts, deep trees
        p = GEO ** np.arange(k)
        body = rng.choice(k, m, p=p / p.sum())
    elif dist == "identical":                       # every group the same 50 symbols: every group cost ties
        body = np.tile(rng.randint(0, k, 50), m // 50 + 1)[:m]
    elif dist == "cycling":                         # four group types on disjoint symbol sets, cycling group by group
        ty = (np.arange(m) // 50) % 4
        r = rng.random_sample(m)
        body = np.minimum(np.floor(-np.log2(np.maximum(r, 1e-12))).astype(np.int64) * 4 + ty, k - 1)
    else:
        raise ValueError(dist)
    return np.append(body, k).astype(np.uint16)


def _block(A, asz, used, seed=0):
    return {"A": A, "asz": int(asz), "used": used, "crc": (0x9E3779B9 * (seed + 1)) & 0xFFFFFFFF, "pidx": (seed * 7919) & 0xFFFFFF}


def _first_bit_diff(a, b, nbits):
    x = np.unpackbits(a)[:nbits]
    y = np.unpackbits(b)[:nbits]
    d = np.nonzero(x != y)[0]
    return int(d[0]) if d.size else None


def _want(oracle, blk):
    ng, sel, lens = oracle.huff_groups(blk["A"], blk["asz"])
    rc, bits, nbits = oracle.bzip2_block_bits(blk["A"], blk["asz"], blk["used"], blk["crc"], blk["pidx"])
    assert rc == 0
    return ng, sel, lens, bits, nbits


def _same(tag, got, want):
    """got / want: (ngroups, selectors, lengths[ng][asz+2], bytes, nbits); names the first difference"""
    ng, sel, lens, bits, nbits = got
    wng, wsel, wlens, wbits, wnbits = want
    assert ng == wng, "%s: %d tables, want %d" % (tag, ng, wng)
    if not np.array_equal(sel, wsel):
        g = int(np.nonzero(sel != wsel)[0][0])
        raise AssertionError("%s: selector %d is %d, want %d (%d differ)" % (tag, g, sel[g], wsel[g], int((sel != wsel).sum())))
    if not np.array_equal(lens, wlens):
        t, s = (int(v[0]) for v in np.nonzero(lens != wlens))
        raise AssertionError("%s: table %d symbol %d has length %d, want %d" % (tag, t, s, lens[t, s], wlens[t, s]))
    d = _first_bit_diff(bits, wbits, min(nbits, wnbits))
    assert d is None, "%s: bit %d of the block differs" % (tag, d)
    assert nbits == wnbits, "%s: %d bits, want %d" % (tag, nbits, wnbits)
    assert np.array_equal(bits, wbits)


def _check(hip, oracle, blk, tag=""):
    want = _want(oracle, blk)
    assert want[0] == _target(blk["A"].size)
    got = {}
    for path in (PER_BLOCK, CHAIN):
        rc, out = hip.stage_huff_blocks([blk], path)
        assert rc == 0, "path %d: rc %d" % (path, rc)
        got[path] = out[0]
        _same("%s path %d" % (tag, path), out[0], want)
    _same("%s path 1 vs path 2" % tag, got[PER_BLOCK], got[CHAIN])
    return want


# ------------------------------------------------------------------ sizes: thresholds and workgroup boundaries
SIZES = [2, 49, 50, 51, 199, 200, 201, 599, 600, 1199, 1200, 2399, 2400, 2401,
         3999, 4000, 4001,                          # one 80-group packing tile
         25550, 25600, 25650,                       # 512-group assign step
         102350, 102400, 102450,                    # 2048 groups per hs_assign workgroup
         131071, 131072, 131073,                    # 131,072 symbols per hs_count workgroup
         899982]                                    # the largest level-9 block
DISTS = ["uniform", "dominant", "zeros", "geometric", "identical", "cycling"]


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("npos", SIZES)
def test_sizes(hip, oracle, npos, dist):
    rng = np.random.RandomState(npos * 7 + DISTS.index(dist))
    asz = (17, 255, 3)[(SIZES.index(npos) + DISTS.index(dist)) % 3]
    blk = _block(_syms(rng, npos, asz, dist), asz, _used(rng, asz, "scattered"), npos)
    _check(hip, oracle, blk, "npos %d %s" % (npos, dist))


# ------------------------------------------------------------------ alphabets and used maps
@pytest.mark.parametrize("kind", ["contiguous", "scattered"])
@pytest.mark.parametrize("asz", [1, 2, 3, 17, 255, 256])
@pytest.mark.parametrize("npos", [700, 30001])
def test_alphabets(hip, oracle, npos, asz, kind):
    rng = np.random.RandomState(asz * 31 + npos + (kind == "scattered"))
    for dist in ("uniform", "geometric"):
        blk = _block(_syms(rng, npos, asz, dist), asz, _used(rng, asz, kind), asz)
        _check(hip, oracle, blk, "asz %d %s %s" % (asz, kind, dist))


# ------------------------------------------------------------------ the length limiter
@pytest.mark.parametrize("npos", [25600, 102401, 131073, 899982])
def test_length_limiter(hip, oracle, npos):
    rng = np.random.RandomState(npos)
    asz = 255
    A = _syms(rng, npos, asz, "geometric")
    freq = np.bincount(A, minlength=asz + 2)
    assert _depth(freq) > 20, "precondition: the global table needs the limiter"
    assert oracle.huff_lengths(freq).max() == 20
    want = _check(hip, oracle, _block(A, asz, _used(rng, asz, "scattered"), 1), "limiter npos %d" % npos)
    assert want[2].max() == 20


# ------------------------------------------------------------------ ties
def test_usage_tie(hip, oracle):
    # half the groups all RUNA (cheapest under the global table), half uniform over the rare ranks (cheapest under the flat
    # one): the first assignment uses both tables equally often, so the table that is split is the first most used one
    asz = 17
    for npos in (2400, 2480, 30000, 139970):         # an even number of groups, the last one of the uniform kind
        nsel = (npos + 49) // 50
        rng = np.random.RandomState(npos)
        sizes = [50] * (nsel - 1) + [npos - 50 * (nsel - 1)]
        A = np.concatenate([np.zeros(n, np.int64) if g % 2 == 0 else rng.randint(2, asz + 1, n) for g, n in enumerate(sizes)])
        A[-1] = asz + 1
        A = A.astype(np.uint16)
        n = asz + 2
        glob = oracle.huff_lengths(np.bincount(A, minlength=n)).astype(np.int64)
        flat = oracle.huff_lengths(np.ones(n, np.uint32)).astype(np.int64)
        gi = np.arange(npos) // 50
        cost = np.stack([np.bincount(gi, weights=t[A], minlength=nsel) for t in (glob, flat)])
        first = np.where(cost[1] < cost[0], 1, 0)
        assert (first == 0).sum() == (first == 1).sum(), "precondition: both tables used equally often"
        _check(hip, oracle, _block(A, asz, _used(rng, asz, "contiguous"), npos), "usage tie npos %d" % npos)


def test_cost_ties_every_group(hip, oracle):
    # every group identical: every cost of every group ties under every table (first minimum; stable median split)
    for npos in (251, 2451, 25601, 102451, 131122):
        rng = np.random.RandomState(npos)
        for asz in (2, 17, 255):
            blk = _block(_syms(rng, npos, asz, "identical"), asz, _used(rng, asz, "scattered"), npos)
            _check(hip, oracle, blk, "identical npos %d asz %d" % (npos, asz))


def test_six_distinct_tables(hip, oracle):
    for npos in (2400, 60000, 300001):
        rng = np.random.RandomState(npos)
        blk = _block(_syms(rng, npos, 255, "cycling"), 255, _used(rng, 255, "scattered"), npos)
        ng, _, lens, _, _ = _check(hip, oracle, blk, "cycling npos %d" % npos)
        assert ng == 6 and len({t.tobytes() for t in lens}) == 6, "precondition: six distinct tables"


# ------------------------------------------------------------------ one call, blocks of every target
@pytest.fixture(scope="module")
def mixed_blocks():
    rng = np.random.RandomState(2024)
    ranges = {2: (2, 199), 3: (200, 599), 4: (600, 1199), 5: (1200, 2399), 6: (2400, 40000)}
    blocks = []
    for t, (lo, hi) in ranges.items():
        for i in range(9):
            npos = int(rng.randint(lo, hi + 1)) if i else lo
            asz = int(rng.choice([1, 2, 3, 17, 60, 255, 256]))
            dist = DISTS[(t + i) % len(DISTS)]
            blocks.append(_block(_syms(rng, npos, asz, dist), asz, _used(rng, asz, ("contiguous", "scattered")[i % 2]), len(blocks)))
    for npos in (102401, 131073, 262145, 899982):   # blocks over several hs_assign / hs_count workgroups beside the short ones
        blocks.append(_block(_syms(rng, npos, 255, "geometric"), 255, _used(rng, 255, "scattered"), len(blocks)))
    order = rng.permutation(len(blocks))
    blocks = [blocks[i] for i in order]
    counts = np.bincount([_target(b["A"].size) for b in blocks], minlength=7)
    assert (counts[2:] >= 8).all(), "precondition: at least 8 blocks of every target"
    return blocks


@pytest.mark.parametrize("path", [PER_BLOCK, CHAIN])
def test_mixed_batch(hip, oracle, mixed_blocks, path):
    rc, out = hip.stage_huff_blocks(mixed_blocks, path)
    assert rc == 0
    for k, blk in enumerate(mixed_blocks):
        _same("block %d (npos %d, asz %d) of the batch" % (k, blk["A"].size, blk["asz"]), out[k], _want(oracle, blk))
        rc, one = hip.stage_huff_blocks([blk], path)
        assert rc == 0
        _same("block %d alone vs in the batch" % k, one[0], out[k])


def test_auto_path_equals_forced(hip, mixed_blocks):
    rc, a = hip.stage_huff_blocks(mixed_blocks, 0)
    rc2, b = hip.stage_huff_blocks(mixed_blocks, CHAIN)
    assert rc == 0 and rc2 == 0
    for k in range(len(mixed_blocks)):
        _same("block %d auto vs chain" % k, a[k], b[k])


def test_stage_rejects_bad_blocks(hip):
    ok = _block(np.array([0, 2, 1, 3], np.uint16), 2, np.array([5, 9], np.uint8))
    assert hip.stage_huff_blocks([ok], CHAIN)[0] == 0
    assert hip.stage_huff_blocks([ok], 3)[0] == -32
    assert hip.stage_huff_blocks([dict(ok, A=np.array([0, 4], np.uint16))], PER_BLOCK)[0] == -32     # symbol > asz + 1
    assert hip.stage_huff_blocks([dict(ok, used=np.array([9, 5], np.uint8))], PER_BLOCK)[0] == -32   # not ascending


# ------------------------------------------------------------------ through the public API: shapes that take the chain
def _cut(oracle, src, level, nfull):
    """nfull full RLE1 blocks of `src` plus a tail block of at most 150 bytes"""
    blocks = oracle.rle1_blocks(src, level)
    assert len(blocks) > nfull
    data = src[: blocks[nfull - 1][3] + 100].copy()
    b = oracle.rle1_blocks(data, level)
    cap = level * 100000 - 19
    assert len(b) == nfull + 1 and all(x[0].size == cap for x in b[:-1]) and b[-1][0].size <= 150
    return data, b


@pytest.fixture(scope="module")
def chain_inputs(oracle):
    p = GEO ** np.arange(60)
    src = np.random.RandomState(1).choice(60, 9100000, p=p / p.sum()).astype(np.uint8)
    out = {}
    for level, nfull in ((9, 10), (1, 88)):
        data, blocks = _cut(oracle, src, level, nfull)
        nb, cap = len(blocks), level * 100000 - 19
        assert 8 <= nb <= 512 and nb * cap >= 8 << 20, "precondition: cjs_bzip2_compress builds the tables on the chain"
        U, pidx = oracle.bwt_cyclic(blocks[-1][0])
        A, _, _ = oracle.mtf_rle2(U, blocks[-1][0])
        assert _target(A.size) == 2, "precondition: the tail block has two tables"
        rc, want = oracle.bzip2_compress(data, level)
        assert rc == 0
        out[level] = (data, blocks, want)
    return out


def test_chain_inputs_reach_the_limiter(oracle, chain_inputs):
    # one 899,981-byte block of the draw has a global table deeper than 20 bits, and final tables with 20-bit codes
    _, blocks, _ = chain_inputs[9]
    deep = 0
    for blk, _, _, _ in blocks[:10]:
        U, _ = oracle.bwt_cyclic(blk)
        A, freq, asz = oracle.mtf_rle2(U, blk)
        d = max(oracle.huff_alloc(sorted(int(x) for x in freq), 32))       # the reference's allocator without the limit
        if d > 20:
            deep += 1
            assert oracle.huff_groups(A, asz)[2].max() == 20
    assert deep >= 1, "precondition: the limiter engages on a global table"


@pytest.mark.parametrize("level", [9, 1])
def test_chain_shape_streams(hip, chain_inputs, level):
    data, _, want = chain_inputs[level]
    rc, got = hip.bzip2_compress(data, level)
    assert rc == 0
    assert got.size == want.size and np.array_equal(got, want), "stream differs from the oracle at byte %s" % (
        np.nonzero(got[: min(got.size, want.size)] != want[: min(got.size, want.size)])[0][:1])
    rc, back = hip.bzip2_decompress(got)
    assert rc == 0 and np.array_equal(back, data)


@pytest.mark.parametrize("level", [9, 1])
def test_chain_shape_batches(oracle, chain_inputs, level):
    import importlib
    pkg = importlib.import_module("compressjs-flattened_amd")
    data, _, want = chain_inputs[level]
    tiny = [np.frombuffer(b"a", np.uint8), np.frombuffer(b"banana", np.uint8), data[:4000].copy()]
    ins = [tiny[0], data, tiny[1], tiny[2]]
    outs = pkg.Bzip2.compressFiles(ins, level)
    assert np.array_equal(outs[1], want)
    for x, o in zip(ins, outs):
        assert np.array_equal(o, oracle.bzip2_compress(x, level)[1])
    backs = pkg.Bzip2.decompressFiles(outs)
    for x, b in zip(ins, backs):
        assert np.array_equal(b, x)
