"""mtf_replay walks its list words in tiers decided per wave (mtf.hip): blocks whose MTF ranks sit on the seams of that form.

The kernel gives one lane to each chunk of 512 run heads (chunk c of a block = lane c mod 64 of wave c div 64; step t of a wave
replays head t of each of its chunks).  The first 64 list positions are 16 registers of four positions each, searched and
shifted in tiers of words (0-3, 4-7, then two at a time) only as far as the deepest lane of the wave needs; positions >= 64
are an LDS row.  What decides the path of a step is therefore the RANK of every lane's head, so the blocks here are built from
rank sequences: every head is a run of length one and has a rank >= 1, which makes the oracle's symbol i exactly
(rank of head i) + 1 -- the generators are checked against that before anything is compared, so a generator that misses its
target fails instead of passing vacuously.  All cases compare `A`, `npos` and `freq` of `cjs_stage_mtf` with the oracle's MTF.
"""
import numpy as np
import pytest

from mtf_cases import heads_from_ranks

CHUNK = 512        # heads per lane (MTF_CHUNK)
WAVE = 64
EXACT_RANKS = [3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65]      # + asz - 1; either side of a word, a tier and the register part
ALPHABETS = [2, 5, 17, 65, 66, 256]


def oracle_side(oracle, U, ranks):
    """the oracle's MTF of one block, after checking that the block has the ranks it was built for"""
    wa, wf, wasz = oracle.mtf_rle2(U, U)
    assert wa.size == ranks.size + 1 and wa[-1] == wasz + 1, "generator: a head with rank 0 or a run longer than one"
    got = wa[:-1].astype(np.int64) - 1
    if not np.array_equal(got, ranks):
        bad = int(np.nonzero(got != ranks)[0][0])
        raise AssertionError("generator: head %d has rank %d, wanted %d" % (bad, got[bad], ranks[bad]))
    return wa, wf, wasz


def check_blocks(hip, oracle, blocks, asz_want=None):
    """blocks: [(U, ranks)]: every block against the oracle; one cjs_stage_mtf call for the blocks of each length (the closing
    heads make lengths differ)"""
    if asz_want is not None:
        assert [oracle_side(oracle, U, ranks)[2] for U, ranks in blocks] == list(asz_want)
    by_len = {}
    for b in blocks:
        by_len.setdefault(b[0].size, []).append(b)
    for _, group in sorted(by_len.items()):
        _check_same_length(hip, oracle, group)


def _check_same_length(hip, oracle, blocks):
    n = blocks[0][0].size
    want = [oracle_side(oracle, U, ranks) for U, ranks in blocks]
    if hip is None:
        return
    allU = np.concatenate([b[0] for b in blocks])
    rc, A, npos, freq, asz = hip.stage_mtf(allU, allU, n)
    assert rc == 0
    for k, (wa, wf, wasz) in enumerate(want):
        assert asz[k] == wasz, "block %d: alphabet %d want %d" % (k, asz[k], wasz)
        assert npos[k] == wa.size, "block %d: npos %d want %d" % (k, npos[k], wa.size)
        got = A[k, :wa.size]
        if not np.array_equal(got, wa):
            bad = np.nonzero(got != wa)[0]
            h = int(bad[0])         # symbol i belongs to head i in these blocks
            raise AssertionError("block %d: %d symbols differ, first at head %d (chunk %d = lane %d of wave %d, head %d of the chunk; "
                                 "rank wanted %d): got symbol %d want %d"
                                 % (k, bad.size, h, h // CHUNK, h // CHUNK % WAVE, h // CHUNK // WAVE, h % CHUNK,
                                    int(blocks[k][1][min(h, blocks[k][1].size - 1)]), got[h], wa[h]))
        if not np.array_equal(freq[k, :wasz + 2], wf):
            bad = int(np.nonzero(freq[k, :wasz + 2] != wf)[0][0])
            raise AssertionError("block %d: freq[%d] = %d want %d" % (k, bad, freq[k, bad], wf[bad]))


# ---- the cases (built without a GPU; `hip` = None only checks the generators against the oracle) ------------------------------
def case_constant_ranks(hip, oracle):
    """every head has rank < 4; every head has rank exactly R (cyclic visits of R + 1 symbols), for each alphabet that has R"""
    n_heads = 3 * CHUNK + 37
    blocks, aszs = [], []
    rng = np.random.default_rng(11)
    for asz in ALPHABETS:
        blocks.append(heads_from_ranks(asz, rng.integers(1, min(4, asz), n_heads).tolist()))
        aszs.append(asz)
        for R in sorted(set(EXACT_RANKS + [asz - 1])):
            if R > asz - 1:         # no such rank in this alphabet
                continue
            U, ranks = heads_from_ranks(asz, [R] * n_heads)
            assert np.all(ranks[:n_heads] == R)
            blocks.append((U, ranks))
            aszs.append(asz)
    assert len(blocks) >= 40
    check_blocks(hip, oracle, blocks, aszs)


DEPTHS = [(8, 11), (36, 47), (60, 70), (100, 255)]      # second tier; the tiers two words wide; across position 64; the LDS row


def case_one_lane_apart(hip, oracle):
    """one chunk of a wave deep and the 63 others shallow, and the reverse; the odd lane being lane 0, 63 and 29"""
    n_heads = WAVE * CHUNK - 256            # room for the closing heads: 64 chunks either way
    rng = np.random.default_rng(12)
    blocks = []
    for lo, hi in DEPTHS:
        for lane in (0, 63, 29):
            for one_deep in (True, False):
                deep = rng.integers(lo, hi + 1, n_heads)
                shallow = rng.integers(1, 4, n_heads)
                is_odd = (np.arange(n_heads) // CHUNK) == lane
                ranks = np.where(is_odd == one_deep, deep, shallow)
                U, r = heads_from_ranks(256, ranks.tolist())
                assert -(-r.size // CHUNK) == WAVE and np.array_equal(r[:n_heads], ranks)
                blocks.append((U, r))
    assert len(blocks) == 24
    check_blocks(hip, oracle, blocks)


def case_chunk_edges(hip, oracle):
    """the deep head is the first and the last head of a chunk; the last chunk is short (H no multiple of 512 nor of 16)"""
    rng = np.random.default_rng(13)
    blocks = []
    for lo, hi in DEPTHS:
        n_heads = 66 * CHUNK + 300 + 7
        ranks = rng.integers(1, 4, n_heads)
        first = np.arange(0, n_heads, CHUNK)
        last = np.minimum(first + CHUNK - 1, n_heads - 1)
        pick = rng.random(first.size) < 0.5
        pick[[0, 1, 63, 64, 65, 66]] = True            # the short chunk (66) among them: its last head is head H - 1
        ranks[first[pick]] = rng.integers(lo, hi + 1, int(pick.sum()))
        ranks[last[pick]] = rng.integers(lo, hi + 1, int(pick.sum()))
        ranks[300:556] = 255                                # every symbol early on: no closing heads, the length is exact
        U, r = heads_from_ranks(256, ranks.tolist())
        assert r.size == n_heads and n_heads % 16 and r[-1] >= lo and r[(n_heads - 1) // CHUNK * CHUNK] >= lo
        blocks.append((U, r))
    check_blocks(hip, oracle, blocks)


def case_chunk_counts(hip, oracle):
    """fewer than 64 chunks, exactly 64, exactly 65 (one head in the last), ranks of every depth"""
    rng = np.random.default_rng(14)
    for n_heads in (10 * CHUNK - 5, 7, CHUNK, 64 * CHUNK, 64 * CHUNK + 1, 65 * CHUNK):
        ranks = np.clip(rng.geometric(1.0 / 12.0, n_heads), 1, 255)
        ranks[:256] = 255                                   # every symbol early on: no closing heads, the length is exact
        if n_heads < 256:
            U, r = heads_from_ranks(n_heads, [n_heads - 1] * n_heads)     # (a tiny block: its own alphabet)
        else:
            U, r = heads_from_ranks(256, ranks.tolist())
        assert r.size == n_heads
        check_blocks(hip, oracle, [(U, r)])


def case_geometric(hip, oracle):
    """300 random blocks, ranks 1 + a geometric law whose mean goes from 1 to 100 over the blocks"""
    rng = np.random.default_rng(15)
    small, large = [], []
    for k in range(300):
        mean = 100.0 ** (k / 299.0)
        big = k % 15 == 7                                   # 20 of them fill more than one wave
        n_heads = 79 * CHUNK + 129 if big else 6 * CHUNK + 451
        asz = (66, 130, 256)[k % 3]
        extra = rng.geometric(1.0 / mean, n_heads) - 1 if mean > 1.0 else np.zeros(n_heads, dtype=np.int64)
        ranks = np.clip(1 + extra, 1, asz - 1)
        ranks[:asz] = asz - 1                               # every symbol early on: exact length
        U, r = heads_from_ranks(asz, ranks.tolist())
        assert r.size == n_heads
        if k in (0, 299):                                   # the sweep does reach both ends (the clip at asz - 1 = 255 costs a little)
            assert (ranks[asz:].mean() < 2.1) if k == 0 else (ranks[asz:].mean() > 80.0)
        (large if big else small).append((U, r))
    assert len(small) == 280 and len(large) == 20
    check_blocks(hip, oracle, small)
    check_blocks(hip, oracle, large)


CASES = [case_constant_ranks, case_one_lane_apart, case_chunk_edges, case_chunk_counts, case_geometric]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_generators_hit_their_ranks(oracle, case):
    # no GPU: every block of every case is built and its ranks are read back from the oracle
    case(None, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_mtf_tiers(hip, oracle, case):
    case(hip, oracle)
