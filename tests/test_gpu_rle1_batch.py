"""The three stage-0 kernels of the batched compressor, each on its own (cjs_stage_rle1_batch): rle_batch_len, rle_batch_walk and
rle_batch_materialize (with the block CRCs as run_sub makes them right behind) over inputs packed back to back.  The reference is
the oracle run on every input alone: the kernels must restart runs and chunks at every input.  The walk and the materialise
kernel both get the ORACLE's tables, so that neither inherits the other's mistake.  Cases: tests/rle1_cases.py, families G, H."""
import numpy as np
import pytest

import rle1_cases as rc

pytestmark = pytest.mark.gpu

INVALID_ARG = -32
FILL = 0xEE
FILL64, FILL32 = 0xEEEEEEEEEEEEEEEE, 0xEEEEEEEE


def run_batch(hip, oracle, key, items, cap, grant=None, canaries=4):
    """one call over `items` [(name, bytes)]: every input through the length kernel, every non-empty input through the walk
    (granted its number of blocks + 1 slots, or grant[name]), every oracle block through the materialise kernel.  Asserts all
    outputs; returns nothing."""
    buf, se = rc.pack(items)
    want = [rc.want(oracle, "%s/%s" % (key, n), d, cap) for n, d in items]
    walk = [k for k, (_, d) in enumerate(items) if d.size]
    slots = [(grant or {}).get(items[k][0], len(want[k]) + 1) for k in walk]
    tbase = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
    mat, owner = [], []
    for k, blocks in enumerate(want):
        for q, (b, _, s, e) in enumerate(blocks):
            mat.append((se[k][0] + s, se[k][0] + e, b.size))
            owner.append((k, q))
    stride = (cap + 15 & ~15) + 16
    r, len2, (ws, we, wl), nblk, rows, crc = hip.stage_rle1_batch(buf, se, cap, walk, tbase.tolist(), int(tbase[-1]) + canaries, mat, stride, FILL)
    assert r == 0, "%s: rc %d" % (key, r)
    # 1. lengths
    for k, (name, d) in enumerate(items):
        E = oracle.rle1_len(d)
        assert int(len2[k]) >> 1 == min(E, cap + 1), "%s/%s: len2 says %d, RLE1 length %d (cap %d)" % (key, name, int(len2[k]) >> 1, E, cap)
        if E <= cap:
            assert int(len2[k]) & 1 == int(rc.absorbed_flag(d)), "%s/%s: absorbed flag %d (length %d, cap %d)" % (key, name, int(len2[k]) & 1, E, cap)
    # 2. the walk
    for j, k in enumerate(walk):
        name, blocks, t0, tcap = items[k][0], want[k], int(tbase[j]), slots[j]
        assert int(nblk[j]) == len(blocks), "%s/%s: walk counts %d blocks, want %d" % (key, name, int(nblk[j]), len(blocks))
        for q in range(tcap):
            got = (int(ws[t0 + q]), int(we[t0 + q]), int(wl[t0 + q]))
            exp = (blocks[q][2], blocks[q][3], blocks[q][0].size) if q < len(blocks) else (FILL64, FILL64, FILL32)
            assert got == exp, "%s/%s: walk slot %d holds (s, e, len) = %s, want %s" % (key, name, q, got, exp)
    for q in range(int(tbase[-1]), int(tbase[-1]) + canaries):
        assert (int(ws[q]), int(we[q]), int(wl[q])) == (FILL64, FILL64, FILL32), "%s: the walk wrote behind the granted slots (%d)" % (key, q)
    # 3. bytes and CRCs
    for j, (k, q) in enumerate(owner):
        b, wcrc = want[k][q][0], want[k][q][1]
        if not np.array_equal(rows[j, : b.size], b):
            bad = np.nonzero(rows[j, : b.size] != b)[0]
            raise AssertionError("%s/%s block %d: %d bytes differ, first at %d (got %d want %d)"
                                 % (key, items[k][0], q, bad.size, bad[0], rows[j, bad[0]], b[bad[0]]))
        rest = np.nonzero(rows[j, b.size:] != FILL)[0]
        assert not rest.size, "%s/%s block %d: row byte %d behind the block's %d was written" % (key, items[k][0], q, b.size + rest[0], b.size)
        assert int(crc[j]) == wcrc, "%s/%s block %d: crc %08x want %08x" % (key, items[k][0], q, int(crc[j]), wcrc)


def test_family_g_batch(hip, oracle):
    cap, items = rc.family_g()
    run_batch(hip, oracle, "g", items, cap, grant={"five_blocks": 2, "len_8193": 1, "len_4097": 3})
    # the same inputs in reverse order (other offsets, other neighbours) and every input granted exactly its blocks
    run_batch(hip, oracle, "g", items[::-1], cap, grant={n: len(rc.want(oracle, "g/" + n, d, cap)) for n, d in items}, canaries=1)


def test_family_h_sweep_as_batches(hip, oracle):
    by_cap = {}
    for i, data, cap in rc.family_h():
        by_cap.setdefault(cap, []).append((i, data))
    for cap, group in sorted(by_cap.items()):
        while group:                                         # (one call materialises at most 65535 blocks: cap 2 makes thousands per input)
            n, blocks = 0, 0
            while n < len(group) and (n == 0 or blocks + len(rc.want(oracle, "h/%d" % group[n][0], group[n][1], cap)) <= 60000):
                blocks += len(rc.want(oracle, "h/%d" % group[n][0], group[n][1], cap))
                n += 1
            part, group = group[:n], group[n:]
            try:
                run_batch(hip, oracle, "h", [("%d" % i, d) for i, d in part], cap, grant={"%d" % part[0][0]: 1})
            except AssertionError as e:
                raise AssertionError("(seed %d, cap %d, indices %s): %s" % (rc.H_SEED, cap, [i for i, _ in part], e))


def test_refusals(hip):
    buf = rc.noise(300)
    se = [(1, 100), (100, 300)]
    ok = dict(item=[0, 1], tbase=[0, 2, 4], mat=[(1, 50, 49)], stride=64)
    assert hip.stage_rle1_batch(buf, se, 50, **ok)[0] == 0
    for cap in (0, 1, 899982):
        assert hip.stage_rle1_batch(buf, se, cap, **ok)[0] == INVALID_ARG, cap
    assert hip.stage_rle1_batch(buf, se, 50, **dict(ok, item=[0, 2]))[0] == INVALID_ARG              # no such input
    assert hip.stage_rle1_batch(buf, se, 50, **dict(ok, tbase=[0, 3, 2]))[0] == INVALID_ARG          # slots run backwards
    assert hip.stage_rle1_batch(buf, se, 50, table_slots=3, **ok)[0] == INVALID_ARG                  # more granted than there are
    assert hip.stage_rle1_batch(buf, [(1, 100), (100, 301)], 50, **ok)[0] == INVALID_ARG             # an input behind the buffer
    assert hip.stage_rle1_batch(buf, [(100, 1), (100, 300)], 50, **ok)[0] == INVALID_ARG
    assert hip.stage_rle1_batch(buf, se, 50, **dict(ok, mat=[(1, 50, 65)]))[0] == INVALID_ARG        # a block longer than its row
    assert hip.stage_rle1_batch(buf, se, 50, **dict(ok, mat=[(1, 301, 49)]))[0] == INVALID_ARG
