"""The MTF stage's run heads, chunk-start lists and RLE2 emission (mtf.hip: mtf_head_count / _scan / _write, mtf_seg_last / _scan,
mtf_chunk_lists, mtf_emit_count / _scan / _write) on blocks that put something on every border of their geometry, through
cjs_stage_mtf_var: blocks of different lengths in slots of one stride, the holes behind them and the whole workspace filled as
the caller says.

The blocks are built from (rank, run length) pairs (mtf_cases.block_from_heads) or, where byte positions matter, from run-start
positions.  Each family has a test without the gpu mark that holds the oracle's MTF against the plain restatement of the expected
output (mtf_cases.expected_from_heads) and asserts that the input puts its seams where the family says, so that a generator that
misses fails instead of passing vacuously; and a gpu test that compares A[:npos], npos, freq[:asz + 2], asz, alist[:asz] and
nheads of every block with the oracle, exactly.
"""
import numpy as np
import pytest

import recipes
from mtf_cases import block_from_heads, expected_from_heads, heads_of, zero_runs

# the geometry of mtf.hip
CHUNK = 512                      # heads per chunk of the replay (MTF_CHUNK)
SEG_CHUNKS = 32                  # chunks per segment of the start lists (MTF_SEG)
SEG = SEG_CHUNKS * CHUNK         # 16384 heads
HEAD_TILE = 16384                # bytes per tile of mtf_head_count / mtf_head_write (HT_TILE)
HEAD_ROUND = 4096                # bytes per round of mtf_head_write
COUNT_PER, WRITE_PER = 16, 4     # bytes per thread of the count pass / of a round of the write pass
EMIT_TILE = 16384                # heads per tile of mtf_emit_count / mtf_emit_write (ET_TILE)
EMIT_ROUND = 4096                # heads per round (MT_TILE)
EMIT_PER = 4                     # heads per thread of a round


# ---- one call, every block against the oracle ------------------------------------------------------------------------------------
_want_memo = {}      # block bytes -> what the oracle says; the calls of a family share blocks


def _want(oracle, U):
    key = U.tobytes()
    if key not in _want_memo:
        wa, wf, wasz = oracle.mtf_rle2(U, U)
        _want_memo[key] = (wa, wf, wasz, np.unique(U), int(np.count_nonzero(U[1:] != U[:-1])) + 1)
    return _want_memo[key]


def _both_references(oracle, U, asz=None, ranks=None, lens=None):
    """the oracle and the restatement agree on one block; (ranks, lens) from the construction, or read back from the bytes"""
    if ranks is None:
        asz, ranks, lens, _ = heads_of(U)
    wa, wf, wasz, walist, wH = _want(oracle, U)
    ea, ef, ealist, eH = expected_from_heads(U, asz, ranks, lens)
    assert wasz == asz, "alphabet: oracle %d, construction %d" % (wasz, asz)
    assert wa.size == ea.size and np.array_equal(wa, ea), "A: oracle and restatement differ (sizes %d / %d)" % (wa.size, ea.size)
    assert np.array_equal(wf, ef), "freq: oracle and restatement differ"
    assert np.array_equal(walist, ealist) and wH == eH


def _where(U, i):
    """symbol i of a block's output: its head and where that head stands in the kernels' geometry"""
    pos = np.flatnonzero(np.concatenate([[True], U[1:] != U[:-1]]))
    lens = np.diff(np.append(pos, U.size))
    lit = np.ones(pos.size, dtype=np.int64)
    lit[0] = 0 if U[0] == U.min() else 1
    z = lens - lit
    cum = np.cumsum(lit + np.frexp((z + 1).astype(np.float64))[1] - 1)
    h = int(min(np.searchsorted(cum, i, side="right"), pos.size - 1))
    p = int(pos[h])
    return ("head %d of %d (run of %d at byte %d: head tile %d, round %d, count thread %d, write thread %d; emit tile %d, round %d, "
            "thread %d; chunk %d, segment %d)"
            % (h, pos.size, lens[h], p, p // HEAD_TILE, p % HEAD_TILE // HEAD_ROUND, p % HEAD_TILE // COUNT_PER, p % HEAD_ROUND // WRITE_PER,
               h // EMIT_TILE, h % EMIT_TILE // EMIT_ROUND, h % EMIT_ROUND // EMIT_PER, h // CHUNK, h // SEG))


def _fills(blocks, hole_fill):
    """hole_fill "last": the hole behind a block repeats the block's last byte"""
    return np.array([b[-1] for b in blocks], dtype=np.uint8) if hole_fill == "last" else hole_fill


def _check_call(hip, oracle, named, stride, hole_fill=0, work_fill=0):
    """one call of cjs_stage_mtf_var over named = [(name, bytes)]; returns {name or (name, slot) for a repeated name: outputs}"""
    blocks = [np.ascontiguousarray(b, dtype=np.uint8) for _, b in named]
    what = "%d blocks, stride %d, holes %s, workspace %#x" % (len(blocks), stride, hole_fill if hole_fill == "last" else hex(hole_fill), work_fill)
    rc, A, npos, freq, asz, alist, nheads = hip.stage_mtf_var(blocks, stride, _fills(blocks, hole_fill), work_fill)
    assert rc == 0, "cjs_stage_mtf_var: %d (%s)" % (rc, what)
    out = {}
    names = [name for name, _ in named]
    for k, (name, U) in enumerate(zip(names, blocks)):
        wa, wf, wasz, walist, wH = _want(oracle, U)
        tag = "block %d (%s, n = %d; %s)" % (k, name, U.size, what)
        assert nheads[k] == wH, "%s: nheads %d want %d" % (tag, nheads[k], wH)
        assert asz[k] == wasz, "%s: alphabet %d want %d" % (tag, asz[k], wasz)
        assert np.array_equal(alist[k, :wasz], walist), "%s: alist %s want %s" % (tag, alist[k, :wasz].tolist(), walist.tolist())
        m = min(int(npos[k]), wa.size)
        if not np.array_equal(A[k, :m], wa[:m]):
            bad = np.flatnonzero(A[k, :m] != wa[:m])
            i = int(bad[0])
            raise AssertionError("%s: %d symbols differ, first symbol %d, %s: got %d want %d" % (tag, bad.size, i, _where(U, i), A[k, i], wa[i]))
        assert npos[k] == wa.size, "%s: npos %d want %d (the first %d symbols agree; symbol %d: %s)" % (tag, npos[k], wa.size, m, m, _where(U, m))
        if not np.array_equal(freq[k, :wasz + 2], wf):
            i = int(np.flatnonzero(freq[k, :wasz + 2] != wf)[0])
            raise AssertionError("%s: freq[%d] = %d want %d" % (tag, i, freq[k, i], wf[i]))
        res = (A[k, :wa.size].copy(), int(npos[k]), freq[k].copy(), int(asz[k]), alist[k, :wasz].copy(), int(nheads[k]))
        out[(name, k) if names.count(name) > 1 else name] = res
    return out


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def _odd(n):
    return n | 1


# ---- a. run lengths and digit counts ---------------------------------------------------------------------------------------------
_A_LENGTHS = sorted({(1 << k) + d for k in range(1, 15) for d in (-1, 0, 1)})      # 1, 2, 3 among them
_A_HEAD0 = (1, 2, 3, 4, 7, 8)
_A_TINY = (b"a", b"aa", b"ab", b"ba", b"aab", b"abb")
_A_ONE_RUN = (899981, (1 << 19) - 1, 1 << 19)      # level 9's block (19 digits); either side of the 19th digit's power of two


def _a_ranks(n, rng):
    r = rng.integers(2, 60, n)
    r[::2] = 1                      # ranks alternate between 1 and deeper
    return r


def _family_a():
    """(small = [(name, U, asz, ranks, lens)] for one call, large = the same for a second call)"""
    rng = np.random.default_rng(201)
    small = []
    lens = rng.permutation(_A_LENGTHS)
    small.append(("every_length",) + _built(64, _a_ranks(lens.size, rng), lens))
    for l0 in _A_HEAD0:            # head 0 of rank 0: its zero run is the whole run
        lens = np.concatenate([[l0], rng.permutation(_A_LENGTHS)])
        ranks = _a_ranks(lens.size, rng)
        ranks[0] = 0
        small.append(("head0_rank0_len%d" % l0,) + _built(64, ranks, lens, True))
    for t in _A_TINY:
        U = np.frombuffer(t, dtype=np.uint8)
        small.append((t.decode(),) + _read_back(U))
    large = [("one_run_%d" % n,) + _built(1, [0], [n], True) for n in _A_ONE_RUN]
    # the powers of two above a small block's reach, each with both neighbours: three runs per block, and 2^19 - 1 as z + 1
    for k in range(15, 19):
        large.append(("runs_2^%d" % k,) + _built(2, [1, 1, 1], [(1 << k) - 1, 1 << k, (1 << k) + 1]))
    large.append(("run_2^19-1",) + _built(2, [1, 1], [(1 << 19) - 1, 1]))
    return small, large


def _built(asz, ranks, lens, first_rank0=False):
    U, r, l = block_from_heads(asz, list(map(int, ranks)), list(map(int, lens)), first_rank0)
    return U, asz, r, l


def _read_back(U):
    asz, ranks, lens, _ = heads_of(U)
    return U, asz, ranks, lens


def test_run_length_blocks_are_what_they_say(oracle):
    small, large = _family_a()
    zp1 = []
    for name, U, asz, ranks, lens in small + large:
        _both_references(oracle, U, asz, ranks, lens)
        zp1 += (zero_runs(ranks, lens) + 1).tolist()
        if name.startswith("head0_rank0"):
            assert ranks[0] == 0 and U[0] == U.min() and zero_runs(ranks, lens)[0] == lens[0] == int(name[15:])
            assert sorted(lens[1:1 + len(_A_LENGTHS)].tolist()) == _A_LENGTHS
        if name == "every_length":
            assert sorted(lens[:len(_A_LENGTHS)].tolist()) == _A_LENGTHS and ranks.min() >= 1
            assert np.all(ranks[0:len(_A_LENGTHS):2] == 1) and np.all(ranks[1:len(_A_LENGTHS):2] > 1)
    zp1 = set(zp1)
    for k in range(1, 20):          # z + 1 on and beside every power of two: where the digit count changes
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= zp1, k
    assert 899982 in zp1 and (899982).bit_length() - 1 == 19
    assert max(U.size for _, U, _, _, _ in small) < 150000


@pytest.mark.gpu
def test_run_lengths_and_digit_counts(hip, oracle):
    small, large = _family_a()
    _check_call(hip, oracle, [(b[0], b[1]) for b in small], _odd(max(b[1].size for b in small)), 0xFF, 0xFF)
    _check_call(hip, oracle, [(b[0], b[1]) for b in large], _A_ONE_RUN[0], 0x00, 0x61)


# ---- b. the next head lives elsewhere --------------------------------------------------------------------------------------------
_B_EXACT_H = (4, 5, 4095, 4096, 4097, 16383, 16384, 16385)


def _b_ranks(H, rng):
    ranks = np.clip(rng.geometric(1.0 / 3.0, H), 1, 255)
    ranks[16:272] = 255             # every symbol early on: no closing heads, H is exact
    return ranks


def _b_long_at(H):
    """the head indexes that carry a long run: the last and the first head of a thread in the middle of a round, either side of a
    round and of a tile of the emit kernels, the last head of the block"""
    return [2051, 6148, EMIT_ROUND - 1, EMIT_ROUND, EMIT_TILE - 1, EMIT_TILE, H - 1]


def _family_b():
    rng = np.random.default_rng(202)
    blocks = []
    for H, long_len in ((38002, 300), (20481, 4097)):
        lens = np.ones(H, dtype=np.int64)
        lens[_b_long_at(H)] = long_len
        blocks.append(("long_runs_%d" % long_len,) + _built(256, _b_ranks(H, rng), lens) + ((H, long_len),))
    for H in _B_EXACT_H:
        lens = rng.integers(1, 6, H)
        lens[-1] = 9
        if H < 256:
            blocks.append(("H_%d" % H,) + _built(H, [H - 1] * H, lens) + ((H, 9),))
        else:
            blocks.append(("H_%d" % H,) + _built(256, _b_ranks(H, rng), lens) + ((H, 9),))
    # one whole emit tile whose heads emit two or more symbols each, between tiles of exactly one symbol per head
    H = 2 * EMIT_TILE + 1100
    lens = np.ones(H, dtype=np.int64)
    lens[EMIT_TILE:2 * EMIT_TILE] = rng.integers(3, 8, EMIT_TILE)
    blocks.append(("uneven_tiles",) + _built(256, _b_ranks(H, rng), lens) + ((H, 1),))
    return blocks


def test_next_head_blocks_are_what_they_say(oracle):
    for name, U, asz, ranks, lens, (H, last_len) in _family_b():
        _both_references(oracle, U, asz, ranks, lens)
        assert ranks.size == H and lens[-1] == last_len and U.size < 150000, name      # H is exact: no closing heads
        if name.startswith("long_runs"):
            assert 16385 <= H <= 40000
            at = _b_long_at(H)
            assert np.all(lens[at] == last_len) and np.count_nonzero(lens != 1) == len(at)
            assert at[0] % EMIT_PER == EMIT_PER - 1 and at[1] % EMIT_PER == 0 and all(0 < a % EMIT_ROUND < EMIT_ROUND - 1 for a in at[:2])
        if name == "uneven_tiles":
            per_head = (ranks > 0) + np.frexp((zero_runs(ranks, lens) + 1).astype(np.float64))[1] - 1
            tiles = [int(per_head[t * EMIT_TILE:(t + 1) * EMIT_TILE].sum()) for t in range(3)]
            assert tiles[0] == EMIT_TILE and tiles[2] == H - 2 * EMIT_TILE and tiles[1] >= 2 * EMIT_TILE and per_head[EMIT_TILE:2 * EMIT_TILE].min() >= 2


@pytest.mark.gpu
def test_next_head_in_another_thread_round_or_tile(hip, oracle):
    blocks = _family_b()
    _check_call(hip, oracle, [(b[0], b[1]) for b in blocks], _odd(max(b[1].size for b in blocks)), 0x00, 0xFF)


# ---- c. byte geometry of head detection ------------------------------------------------------------------------------------------
_C_SYMS = np.array([0x00, 0x61, 0x62, 0x7F, 0x80, 0xFF, 0x0A, 0x20], dtype=np.uint8)
_C_MODULI = (WRITE_PER, COUNT_PER, HEAD_ROUND, HEAD_TILE)


def _geom_block(n, offs, first, last, seed):
    """n bytes whose runs start at `offs` around multiples of 4, 16, 4096 and 16384 (all multiples of 4096, a random choice of the
    others) and at scattered other places; the block starts with the byte `first` and ends with `last`"""
    rng = np.random.default_rng(seed)
    starts = {0}
    for m, p in ((HEAD_ROUND, 1.0), (COUNT_PER, 0.08), (WRITE_PER, 0.02)):
        ms = np.arange(m, n + 2, m)
        for M in ms[rng.random(ms.size) < p].tolist():
            starts.update(M + d for d in offs)
    starts.update(np.flatnonzero(rng.random(n) < 0.01).tolist())
    starts.add(n // 2)
    if n > 30000:       # one run over more than two whole rounds of the write pass
        starts -= set(range(20002, 20002 + 9000))
    starts = np.array(sorted(s for s in starts if 0 <= s < n), dtype=np.int64)
    while True:         # run symbols: neighbours differ; relabelled so that the ends are as asked
        idx = np.cumsum(rng.integers(1, _C_SYMS.size, starts.size)) % _C_SYMS.size
        if (idx[0] == idx[-1]) == (first == last):
            break
    relabel = [first] + ([last] if last != first else []) + [s for s in _C_SYMS.tolist() if s not in (first, last)]
    order = [int(idx[0])] + ([int(idx[-1])] if last != first else []) + [i for i in range(_C_SYMS.size) if i not in (idx[0], idx[-1])]
    table = np.zeros(_C_SYMS.size, dtype=np.uint8)
    table[order] = relabel
    U = np.repeat(table[idx], np.diff(np.append(starts, n)))
    assert U.size == n and U[0] == first and U[-1] == last
    return U, starts


def _family_c(stride, rotate):
    """[(name, U, run starts)], each block starting with the byte the block in front ends with (the last one leads back to the
    first); four copies of one block in consecutive slots; a block that fills its slot, so that the next one starts right behind it"""
    plan = [("phase_-1", 40000, (-1,), 0x62, 0x00), ("phase_0", 39997, (0,), 0x00, 0xFF), ("phase_+1", 39998, (1,), 0xFF, 0x61)]
    plan += [("all_phases", 39999, (-1, 0, 1), 0x61, 0x61)] * 4
    plan += [("n_16383", 16383, (-1, 0, 1), 0x61, 0x00), ("n_16384", 16384, (-1, 0, 1), 0x00, 0xFF), ("n_16385", 16385, (-1, 0, 1), 0xFF, 0x7F),
             ("full_slot", stride, (-1, 0, 1), 0x7F, 0x80), ("behind_full_slot", 37, (0,), 0x80, 0x62)]
    blocks = [(name,) + _geom_block(n, offs, f, l, 300 + n % 97) for name, n, offs, f, l in plan]
    return blocks[rotate:] + blocks[:rotate]


_C_CALLS = [(40001, 0), (40016, 1)]     # slots at all four alignments mod 4; slots 16-aligned (and a block of 0x00 first in the array)


def test_byte_geometry_blocks_are_what_they_say(oracle):
    for stride, rotate in _C_CALLS:
        blocks = _family_c(stride, rotate)
        for name, U, starts in blocks:
            _both_references(oracle, U)
            assert np.array_equal(heads_of(U)[3], starts), name
        for m in _C_MODULI:      # runs begin (and the runs in front of them end) at -1, 0, +1 around the multiples
            assert {m - 1, 0, 1} <= set(np.concatenate([s[1:] for _, _, s in blocks]) % m), m
            assert {m - 1, 0, 1} <= set(np.concatenate([s[1:] for n_, _, s in blocks if n_.startswith("phase")]) % m), m
        assert {U.size % 4 for _, U, _ in blocks} == {0, 1, 2, 3} and {16383, 16384, 16385, stride} <= {U.size for _, U, _ in blocks}
        for (_, U, _), (_, V, _) in zip(blocks, blocks[1:] + blocks[:1]):
            assert V[0] == U[-1]         # with holes that repeat the last byte, and behind the full slot: no change of byte at p == 0
        names = [b[0] for b in blocks]
        k = names.index("all_phases")
        assert names[k:k + 4] == ["all_phases"] * 4 and names[names.index("full_slot") + 1] == "behind_full_slot"
        assert {(j * stride) % 4 for j in range(k, k + 4)} == ({0, 1, 2, 3} if stride % 2 else {0})
        assert {b[1][0] for b in blocks} >= {0x00, 0xFF}
        assert any(np.diff(np.append(s, U.size)).max() > 2 * HEAD_ROUND for _, U, s in blocks)
    assert _family_c(40016, 1)[0][1][0] == 0x00      # the very first byte of the array equals the zero the kernels put in front of it


@pytest.mark.gpu
def test_byte_geometry_of_head_detection(hip, oracle):
    seen = {}
    for stride, rotate in _C_CALLS:
        blocks = _family_c(stride, rotate)
        for hole_fill, work_fill in ((0x00, 0xFF), (0xFF, 0x61), ("last", 0x00)):
            out = _check_call(hip, oracle, [(b[0], b[1]) for b in blocks], stride, hole_fill, work_fill)
            for key, res in out.items():
                name = key[0] if isinstance(key, tuple) else key
                if name == "full_slot":
                    continue                                   # (its length follows the stride)
                first = seen.setdefault(name, res)
                assert _same(first, res), "block %s differs between slots, alignments or fills (stride %d, holes %s)" % (key, stride, hole_fill)
    assert len(seen) == 8


# ---- d. start lists across segments ----------------------------------------------------------------------------------------------
def _d_named_heads(H):
    last_chunk = (H - 1) // CHUNK * CHUNK
    return {"last head of segment 0": SEG - 1, "first head of segment 1": SEG, "last head of chunk 0 of segment 1": SEG + CHUNK - 1,
            "first head of the last chunk": last_chunk}


def _seg_block(asz, H, seed):
    """ranks 1..3 over the first segment; deep ranks at the seams; a few new symbols on the way; the rest of the alphabet first
    seen in the last, short chunk"""
    rng = np.random.default_rng(seed)
    top = min(3, asz - 1)
    ranks = rng.integers(1, top + 1, H)
    deep = lambda: int(rng.integers(min(200, asz - 1), asz))
    for h in _d_named_heads(H).values():
        ranks[h] = deep()
    if asz > 200:
        ranks[rng.choice(np.arange(SEG + CHUNK, 2 * SEG - 1), 60, replace=False)] = [deep() for _ in range(60)]      # new symbols inside segment 1
        ranks[2 * SEG - 1], ranks[2 * SEG] = deep(), deep()                                                           # and at the next seam
    last_chunk = (H - 1) // CHUNK * CHUNK
    ranks[last_chunk + 1:last_chunk + 1 + min(asz, 200)] = asz - 1      # whatever was never seen comes in here, in descending byte order
    return _built(asz, ranks, np.ones(H, dtype=np.int64))


def _head0_once_block():
    """head 0's symbol never comes back inside segment 0, and the byte value 0 is first seen in segment 1: at the start of segment
    1 the oldest seen symbol (last head index 0) stands right in front of the smallest never-seen one.  Both then occur in the
    first chunk of segment 1."""
    rng = np.random.default_rng(44)
    H = 2 * SEG + CHUNK + 40
    s = np.empty(H, dtype=np.int64)
    s[0] = 3
    s[1:SEG] = np.tile([1, 2], SEG)[:SEG - 1]
    s[SEG - 1] = 77
    body = np.cumsum(rng.integers(1, 6, H - SEG)) % 6 + 100                      # six symbols, neighbours differ
    s[SEG:] = body
    s[SEG:SEG + 5] = [200, 0, 3, 0, 201]
    s[2 * SEG - 1:2 * SEG + 2] = [0, 3, 250]
    s[-30:] = np.arange(220, 250)
    s[np.flatnonzero(s[1:] == s[:-1]) + 1] = 99                                   # (the fixed values beside the random ones)
    U = s.astype(np.uint8)
    assert np.all(U[1:] != U[:-1])
    return _read_back(U)


def _family_d():
    H = 2 * SEG + 2 * CHUNK + 300
    return [("asz_256", H) + _seg_block(256, H, 41), ("asz_65", H) + _seg_block(65, H, 42), ("asz_2", H) + _seg_block(2, H, 43),
            ("head0_once", 2 * SEG + CHUNK + 40) + _head0_once_block()]


def test_segment_blocks_are_what_they_say(oracle):
    for name, H, U, asz, ranks, lens in _family_d():
        _both_references(oracle, U, asz, ranks, lens)
        assert ranks.size == H == U.size and H > 2 * SEG + CHUNK and (H - 1) // SEG == 2 and H % CHUNK, name      # reaches segment 2; a short chunk
        syms = U.tolist()
        seen0, seen1 = len(set(syms[:SEG])), len(set(syms[:2 * SEG]))
        last_chunk = (H - 1) // CHUNK * CHUNK
        new_at_end = len(set(syms[last_chunk:]) - set(syms[:last_chunk]))
        if name.startswith("asz_"):
            assert asz == int(name[4:])
            lo = min(200, asz - 1)
            for what, h in _d_named_heads(H).items():
                assert lo <= ranks[h] <= asz - 1, (name, what, ranks[h])
            assert ranks[:SEG - 1].max() <= 3
        if name == "asz_256":
            # segment 0: four symbols under ranks 1..3 and the deep head at its end; segment 1: its two named heads, 60 new symbols on
            # the way, the head at its end; then the first head of segment 2, and everything else in the last chunk
            assert (seen0, seen1, new_at_end) == (5, 68, 256 - 69), (seen0, seen1, new_at_end)
        elif name == "asz_65":
            assert seen0 == 5 and seen1 <= 8 and new_at_end >= 50, (seen0, seen1, new_at_end)
        elif name == "asz_2":
            assert seen0 == seen1 == 2
        else:
            assert syms.index(0) == SEG + 1 and syms[0] == 3 and 3 not in syms[1:SEG] and syms[SEG + 2] == 3 and min(syms) == 0
            assert new_at_end >= 30
        # the head right in front of a segment start is the last occurrence of its symbol before that start
        for s0 in (SEG, 2 * SEG):
            assert max(i for i in range(s0) if syms[i] == syms[s0 - 1]) == s0 - 1


@pytest.mark.gpu
def test_start_lists_across_segments(hip, oracle):
    blocks = _family_d()
    for work_fill in (0x00, 0xFF):
        _check_call(hip, oracle, [(b[0], b[2]) for b in blocks], _odd(max(b[2].size for b in blocks)), 0x00, work_fill)


# ---- e. lengths, holes and a stale workspace -------------------------------------------------------------------------------------
_E_STRIDE = 100000 - 19      # the pipeline's slot at level 1: odd


def _exact_heads(H, seed):
    rng = np.random.default_rng(seed)
    if H == 1:
        return _built(1, [0], [5000], True)[0]
    if H < 256:
        return _built(H, [H - 1] * H, rng.integers(1, 4, H))[0]
    return _built(256, _b_ranks(H, rng), rng.integers(1, 4, H))[0]


def _family_e():
    """{name: bytes}; 0x61 is a byte value that the blocks use (the text blocks and the short ones)"""
    b = {"len_%d" % n: recipes.textgen(n, 500 + n % 89) for n in (1, 2, 3, 15, 16, 17, _E_STRIDE, _E_STRIDE - 1, _E_STRIDE - 15)}
    b["a_x16"] = np.full(16, 0x61, np.uint8)
    b["a_x17"] = np.full(17, 0x61, np.uint8)
    b["ends_with_a"] = np.concatenate([recipes.textgen(30000, 77), np.full(40, 0x61, np.uint8)])
    for H in (1, 511, 512, 513, 16385):
        b["H_%d" % H] = _exact_heads(H, 600 + H)
    b["family_a"] = _family_a()[0][0][1]
    b["family_a_head0"] = _family_a()[0][3][1]
    b["family_b"] = _family_b()[1][1]
    b["family_d"] = _family_d()[0][2]
    b["text_7000"] = recipes.textgen(7000, 79)
    b["text_7000_again"] = b["text_7000"].copy()
    b["family_b_again"] = b["family_b"].copy()
    return b


def test_length_blocks_are_what_they_say(oracle):
    b = _family_e()
    assert 24 <= len(b) <= 26 and max(x.size for x in b.values()) == _E_STRIDE
    assert {1, 2, 3, 15, 16, 17, _E_STRIDE, _E_STRIDE - 1, _E_STRIDE - 15} <= {x.size for x in b.values()}
    for name, U in b.items():
        _both_references(oracle, U)
        if name.startswith("H_"):
            assert heads_of(U)[1].size == int(name[2:]), name
    assert all(0x61 in b[k] for k in ("len_%d" % _E_STRIDE, "a_x16", "ends_with_a", "text_7000")) and b["ends_with_a"][-1] == 0x61
    assert b["H_1"].size == 1 or np.all(b["H_1"] == b["H_1"][0])


@pytest.mark.gpu
def test_lengths_holes_and_a_stale_workspace(hip, oracle):
    """twelve calls over the same blocks: by descending length (the order of the batch compressor) and shuffled, holes of 0x00 and
    0xFF, the workspace filled with 0x00, 0xFF and 0x61; every call against the oracle, and every block the same in all of them
    and at both its slots"""
    b = _family_e()
    names = sorted(b)
    by_len = sorted(names, key=lambda k: -b[k].size)
    shuffled = [names[i] for i in np.random.default_rng(7).permutation(len(names))]
    assert by_len != shuffled
    first = None
    for order_name, order in (("descending", by_len), ("shuffled", shuffled)):
        for hole_fill in (0x00, 0xFF):
            for work_fill in (0x00, 0xFF, 0x61):
                try:
                    got = _check_call(hip, oracle, [(k, b[k]) for k in order], _E_STRIDE, hole_fill, work_fill)
                except AssertionError as e:
                    raise AssertionError("%s order: %s" % (order_name, e))
                first = first or got
                for k in names:
                    assert _same(got[k], first[k]), "block %s differs between calls (%s, holes %#x, workspace %#x)" % (k, order_name, hole_fill, work_fill)
                for k in ("text_7000", "family_b"):
                    assert _same(got[k], got[k + "_again"]), (k, order_name, hole_fill, work_fill)


@pytest.mark.gpu
def test_a_short_call_behind_a_long_one(hip, oracle):
    """the way the product runs: one process, a call over long blocks and then one over short ones"""
    b = _family_e()
    long_set = [(k, b[k]) for k in sorted(b) if b[k].size >= 30000]
    short_set = [(k, b[k]) for k in sorted(b) if b[k].size < 1000]
    assert len(long_set) >= 6 and len(short_set) >= 8
    _check_call(hip, oracle, long_set, _E_STRIDE, 0xFF, 0x61)
    _check_call(hip, oracle, short_set, 1008, 0xFF, 0x61)


# ---- f. the entry point's argument checks ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stage_refuses_what_it_cannot_take(hip):
    ok = [b"nnbaaa", b"ba"]
    for blocks, stride in ((ok, 0), (ok, 5), ([b"nnbaaa", b""], 16), ([np.zeros(17, np.uint8)], 16), ([], 16), ([b"a"] * 65536, 1),
                           ([b"a"], 4096 * 1024 + 1)):
        res = hip.stage_mtf_var(blocks, stride, 0x00, 0xFF)
        assert res[0] == -32 and all(x is None for x in res[1:]), (len(blocks), stride, res[0])      # CJS_E_INVALID_ARG
    for stride in (6, 7, 16):
        rc, A, npos, freq, asz, alist, nheads = hip.stage_mtf_var(ok, stride, 0x61, 0xFF)
        assert rc == 0 and npos.tolist() == [6, 3] and asz.tolist() == [3, 2] and nheads.tolist() == [3, 2]
        assert A[0, :6].tolist() == [3, 0, 3, 3, 1, 4] and freq[0, :5].tolist() == [1, 1, 0, 3, 1] and bytes(alist[0, :3]) == b"abn"
        assert A[1, :3].tolist() == [2, 2, 3] and freq[1, :4].tolist() == [0, 0, 2, 1] and bytes(alist[1, :2]) == b"ab"
