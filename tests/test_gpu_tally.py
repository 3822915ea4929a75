"""The key tally on the GPU (cjs_keys_tally[_device], csrc/tally.hip) against the host rule cjs_stage_keys_tally, which
test_tally_host.py and tests/host/tally_plan_check.cc hold against restatements: made-up key arrays at the sizes where a stage can
break (a radix tile of 4096, the sorter's extra tile per 64 Ki keys, 256 tiles where the sorter's scan changes its form, the
1024-slot tiles of the tally's own kernels), in the shapes that tell a sort by the whole record from a sort by the hash, under
both orders, the filters and short caps between canaries."""
import ctypes
import importlib

import numpy as np
import pytest

import tally_cases as tc

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 1048576, 1048577)
N = 3 * 4096 + 1024 + 17          # the shapes: four radix tiles, the last one short; 13 whole tiles of the tally's kernels and one short


@pytest.fixture(scope="module")
def L():
    return tc.bind()


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def keys_of(hash_, len_, check):
    a = np.zeros(len(hash_), dtype=tc.KEY)
    a["hash"], a["len"], a["check"] = hash_, len_, check
    return a


def skewed(rng, n, pool, bad_share=0.0):
    """n keys drawn with weights 1/k from `pool` random records, a share of them bad"""
    vals = keys_of(rng.randint(0, 2 ** 61 - 1, pool, dtype=np.uint64), rng.randint(1, 200, pool), rng.randint(0, 2 ** 32, pool, dtype=np.uint64))
    w = 1.0 / np.arange(1, pool + 1)
    a = vals[rng.choice(pool, size=n, p=w / w.sum())]
    a[rng.rand(n) < bad_share] = tc.ONES
    return a


def agree(L, torch, keys, order=tc.BY_COUNT, lo=1, hi=0, cap=None, forms=("host", "device"), shift=0):
    """both GPU forms give what the host rule gives, byte for byte, and write nothing else -> (groups, info)"""
    rc, want, winfo = tc.stage_tally(L, keys, order, lo, hi, cap)
    assert rc == 0
    for form in forms:
        if form == "host":
            rc, got, info = tc.host_tally(L, keys, order, lo, hi, cap)
        else:
            rc, got, info = tc.device_tally(L, torch, keys, order, lo, hi, cap, shift=shift)
        assert rc == 0, (form, rc)
        assert tc.info_tuple(info) == tc.info_tuple(winfo), (form, order, lo, hi, tc.info_tuple(info), tc.info_tuple(winfo))
        if got.tobytes() != want.tobytes():
            k = int(np.nonzero(got != want)[0][0])
            raise AssertionError((form, order, lo, hi, cap, "group %d" % k, got[k], want[k]))
    return want, winfo


@pytest.mark.parametrize("n", SIZES)
def test_primitive_sizes(L, torch, n):
    rng = np.random.RandomState(n % 9973 + 5)
    keys = skewed(rng, n, 200 if n < 100000 else 50000, bad_share=0.01)
    want, info = agree(L, torch, keys, tc.BY_COUNT)
    assert int(want["count"].sum()) == n - info.n_bad
    agree(L, torch, keys, tc.BY_FIRST, lo=2, forms=("device",) if n > 100000 else ("host", "device"))


def _shapes():
    rng = np.random.RandomState(99)
    idx = np.arange(N)
    one = lambda v: np.full(N, v, np.uint64)
    out = {}
    out["all equal"] = keys_of(one(12345), one(7), one(9))
    out["all distinct"] = keys_of(rng.permutation(N).astype(np.uint64) * 1000003, one(7), one(9))
    out["two values alternating"] = keys_of(np.where(idx & 1, 5, 2 ** 60 + 5).astype(np.uint64), one(7), one(9))
    out["a skewed draw from 200 values"] = skewed(rng, N, 200)
    pick = rng.randint(0, 2, N).astype(np.uint64)
    out["only the check differs"] = keys_of(one(77), one(7), 9 + pick)
    out["only the check's top bit differs"] = keys_of(one(77), one(7), pick << np.uint64(31))
    out["only the length differs"] = keys_of(one(77), 7 + pick, one(9))
    out["only bit 0 of the hash differs"] = keys_of(77 ^ pick, one(7), one(9))
    out["only bit 60 of the hash differs"] = keys_of(77 + (pick << np.uint64(60)), one(7), one(9))
    # one hash under three (len, check) pairs, interleaved, among records of a lower and a higher hash: a sort by the hash alone
    # leaves the three mixed, and only a stable one keeps every group's first occurrence at its head
    three = np.array([(5, 9), (4, 10), (6, 8)], np.uint64)[rng.randint(0, 3, N)]
    h = np.where(idx % 5 == 0, 10, np.where(idx % 5 == 1, 30, 20)).astype(np.uint64)
    out["one hash, three len/check pairs interleaved"] = keys_of(h, three[:, 0], three[:, 1])
    for name, where in (("bad records at the front", idx < 300), ("bad records at the end", idx >= N - 300), ("bad records scattered", rng.rand(N) < 0.2),
                        ("only bad records", idx >= 0)):
        a = skewed(rng, N, 50)
        a[where] = tc.ONES
        out[name] = a
    # every value three times: all counts tie, the order by count falls back on the first occurrence
    out["count ties"] = keys_of(rng.permutation(np.repeat(np.arange(N // 3 + 1, dtype=np.uint64), 3)[:N]) + 1000, one(1), one(2))
    # sorted by the record, the groups' heads fall on the first and the last slot of the tally's tiles (1024) and of the sorter's
    # (4096): runs of 1023, 1, 1, 3070, 1, 1, 1, ... by ascending hash, shuffled
    runs = [1023, 1, 1, 3070, 1, 1, 1, 1022, 1, 1024, 1, 2047, 1]
    runs.append(N - sum(runs))
    heads = np.cumsum([0] + runs[:-1])
    assert N - sum(runs[:-1]) > 0 and {1023, 1024, 4095, 4096, 5120}.issubset(set(heads.tolist()))
    out["heads on tile borders"] = keys_of(rng.permutation(np.repeat(np.arange(len(runs), dtype=np.uint64) * 3 + 1, runs)), one(1), one(2))
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_primitive_shapes(L, torch, name):
    keys = SHAPES[name]
    for order in (tc.BY_COUNT, tc.BY_FIRST):
        want, info = agree(L, torch, keys, order)
        assert int(want["count"].sum()) == N - info.n_bad
        # (the host rule itself against the restatement that groups the tuples, on this very shape)
        ref, rinfo = tc.tally_ref(list(zip(keys["hash"].tolist(), keys["len"].tolist(), keys["check"].tolist())), order)
        assert tc.info_tuple(info) == rinfo and tc.groups_as_tuples(want) == ref


def test_primitive_calls_filters_and_caps(L, torch):
    rng = np.random.RandomState(3)
    keys = skewed(rng, N, 3000, bad_share=0.02)          # counts from 1 to the hundreds: every filter keeps some and drops some
    for order in (tc.BY_COUNT, tc.BY_FIRST):
        for lo, hi in ((2, 0), (1, 1), (2, 3), (0, 0), (10 ** 6, 0)):
            want, info = agree(L, torch, keys, order, lo, hi)
            assert (info.n_groups == 0) == (lo == 10 ** 6) and (info.n_groups < info.n_distinct) == ((lo, hi) != (0, 0))
            for cap in (0, 1, max(int(info.n_groups) - 1, 0), int(info.n_groups)):
                agree(L, torch, keys, order, lo, hi, cap=cap)


def test_device_keys_at_an_address_that_is_no_multiple_of_16_are_served_and_of_8_refused(L, torch):
    keys = skewed(np.random.RandomState(4), 5000, 100, bad_share=0.01)
    agree(L, torch, keys, forms=("device",), shift=8)
    rc, _, _ = tc.device_tally(L, torch, keys, shift=4)
    assert rc == tc.E_INVALID


def test_the_device_form_refuses_host_memory(L):
    keys = skewed(np.random.RandomState(4), 64, 10)
    out = np.zeros(64, dtype=tc.TALLY)
    info = tc.TallyInfo()
    assert L.cjs_keys_tally_device(keys.ctypes.data, 64, tc.BY_COUNT, 1, 0, out.ctypes.data, 64, ctypes.byref(info), None) == tc.E_INVALID


def test_the_python_front(L, torch):
    pkg = importlib.import_module("compressjs-flattened_amd")
    keys = skewed(np.random.RandomState(8), 6000, 300, bad_share=0.01)
    tuples = list(zip(keys["hash"].tolist(), keys["len"].tolist(), keys["check"].tolist()))
    for order, code in (("count", tc.BY_COUNT), ("first", tc.BY_FIRST)):
        for kw, lo, hi in (({}, 1, 0), ({"min_count": 2}, 2, 0), ({"max_count": 1}, 1, 1)):
            ref, rinfo = tc.tally_ref(tuples, code, lo, hi)
            for limit in (None, 10, 0):
                res = pkg.tally_keys(keys, order=order, limit=limit, **kw)
                assert (res.n_lines, res.n_bad_lines, res.n_distinct, res.n_groups, res.max_count) == rinfo
                assert tc.groups_as_tuples(res.groups) == ref[:limit]


# ---------------------------------------------------------------- the stream tally (cjs_bzip2_tally[_device], whole lines)
import hashlib
import json
import os
import re
import subprocess
import sys

import linekeys_cases as lk
import lines_cases as lc
import range_cases as rg

STREAMS = ("TL1", "CT2", "CT3")
SEEDS = (0, 0xFEEDFACE12345678)


@pytest.fixture(scope="module")
def fx(L, oracle):
    return {name: tc.stream_fixture(L, name, oracle) for name in STREAMS}


def test_the_fixtures_hold_what_the_join_can_get_wrong(fx):
    f = fx["TL1"]
    p = tc.tl1_planted(f["plain"], f["bounds"])
    assert len(f["entries"]) == 4 and 290 * 1024 < f["total"] < 310 * 1024
    assert sorted(x[1] for x in p["seam"]) == [False, True], "one line across a block seam, its twin inside a block"
    assert sorted(x[1:] for x in p["tile"]) == [(False, False), (True, False)], "one line across a tile seam inside a block, its twin inside a tile"
    assert len(p["big"]) == 2 and all(n >= 2 for _, n, _ in p["big"]) and sorted(x[2] for x in p["big"]) == [False, True], "a 40 KiB line twice, once over a block seam"
    assert len(p["empty"]) >= 10 and p["tail"] and len(p["tail_twins"]) >= 1, "repeated empty lines; an unterminated tail equal to earlier lines"
    c = fx["CT2"]
    assert len([e for e in c["entries"] if e[2]]) == 639 and max(lc.blocks_of_line(c["nl"], c["total"], c["bounds"], k) for k in range(c["nl"].size)) >= 13
    assert len(fx["CT3"]["entries"]) == 0
    # a table by records can be held against a table by content: no two distinct lines of a fixture share a record
    for g in fx.values():
        assert tc.distinct_lines_have_distinct_records(g["plain"], SEEDS)


def _windows(f):
    N = int(f["nl"].size)
    if f["name"] == "TL1":
        seam = next(k for k, across in tc.tl1_planted(f["plain"], f["bounds"])["seam"] if across)
        return [(0, None), (5, 1000), (seam, 1), (seam - 1, 3), (N - 2, None), (N, None), (N + 1, None), (0, N)]
    return [(0, None), (N // 3, N // 2), (N, None)]


@pytest.mark.parametrize("name", STREAMS)
def test_stream_tally_against_the_lines(L, fx, name):
    f = fx[name]
    for first, count in _windows(f):
        kw = dict(first=first, count=tc.M64 if count is None else count)
        for i, (order, lo, hi, cap) in enumerate(((tc.BY_COUNT, 1, 0, None), (tc.BY_FIRST, 1, 0, None), (tc.BY_COUNT, 2, 0, 16), (tc.BY_FIRST, 1, 1, None),
                                                 (tc.BY_FIRST, 2, 3, 5))):
            if name == "CT2" and (first or i in (1, 3)) and i != 2:
                continue          # (639 blocks a call: the whole stream under three settings, the windows under one)
            seed = SEEDS[i & 1]
            groups, info = tc.both_forms(L, f, seed=seed, order=order, min_count=lo, max_count=hi, cap=cap, **kw)
            tc.check_against_the_lines(groups, info, f["plain"], seed, first, count, order, lo, hi, cap)
    if name == "TL1":          # the planted lines are one group each with their twins
        groups, info = tc.both_forms(L, f, order=tc.BY_FIRST)
        by_first = {int(g["first"]): int(g["count"]) for g in groups}
        p = tc.tl1_planted(f["plain"], f["bounds"])
        assert by_first[min(k for k, _ in p["seam"])] == 2 and by_first[min(k for k, _, _ in p["tile"])] == 2 and by_first[min(k for k, _, _ in p["big"])] == 2
        assert by_first[p["empty"][0]] == len(p["empty"]) and by_first[p["tail_twins"][0]] == len(p["tail_twins"]) + 1
    if name == "CT3":
        assert tc.stream_info_tuple(info) == (0, 0, 0, 0, 0, 0, 0, tc.M64)


def test_the_python_front_of_the_stream_tally(fx):
    pkg = importlib.import_module("compressjs-flattened_amd")
    f = fx["TL1"]
    ix = pkg.Bzip2Index.build(f["stream"])
    ln = pkg.Bzip2Lines.build(f["stream"], ix)
    ref, rinfo = tc.tally_ref(tc.window_lines(f["plain"]), tc.BY_COUNT, bad=None)
    res = ix.tally_lines(f["stream"], ln, limit=16)
    dev = pkg.tally_lines_device(f["dev"][1], f["stream"].size, ix, ln, limit=16)
    for r in (res, dev):
        assert (r.n_lines, r.n_bad_lines, r.n_distinct, r.n_groups, r.max_count) == (rinfo[0], 0) + rinfo[2:] and r.bad_blocks == 0
        assert [(int(g["first"]), int(g["count"])) for g in r.groups] == [(a, c) for _, a, c in ref[:16]]
    # every group's first line, read back through read_lines in one call
    assert res.text(ix, f["stream"], ln) == b"".join(b"%7d %s\n" % (c, item) for item, _, c in ref[:16])
    # the tally of a cut, and its text through cut_text
    items = tc.cut_window_lines(f["plain"], tc.FIELDS, 9, [(2, 2)])
    cref, cinfo = tc.tally_ref(items, tc.BY_COUNT, bad=None)
    for r in (ix.tally_lines(f["stream"], ln, fields="2", limit=12), pkg.tally_lines_device(f["dev"][1], f["stream"].size, ix, ln, fields=[2], limit=12)):
        assert (r.n_lines, r.n_distinct, r.n_groups, r.max_count) == (cinfo[0],) + cinfo[2:]
        assert [(int(g["first"]), int(g["count"])) for g in r.groups] == [(a, c) for _, a, c in cref[:12]]
        assert r.text(ix, f["stream"], ln) == b"".join(b"%7d %s\n" % (c, item) for item, _, c in cref[:12])
    by_bytes = ix.tally_lines(f["stream"], ln, bytes="1-8", order="first", limit=3)
    assert by_bytes.text(ix, f["stream"], ln) == b"".join(b"%7d %s\n" % (c, item) for item, _, c in tc.tally_ref(tc.cut_window_lines(f["plain"], tc.BYTES, 0, [(1, 8)]), tc.BY_FIRST, bad=None)[0][:3])
    everything = ix.tally_lines(f["stream"], ln, order="first", min_count=2)
    want, _ = tc.tally_ref(tc.window_lines(f["plain"]), tc.BY_FIRST, 2, bad=None)
    assert [(int(g["first"]), int(g["count"])) for g in everything.groups] == [(a, c) for _, a, c in want]


def _digest(groups, info):
    return [hashlib.sha256(groups.tobytes()).hexdigest(), list(tc.stream_info_tuple(info))]


def _digests(L, f):
    N = int(f["nl"].size)
    return [_digest(*tc.both_forms(L, f, seed=SEEDS[1])), _digest(*tc.both_forms(L, f, first=N // 3, count=N // 2, order=tc.BY_FIRST, min_count=2, cap=50))]


def child(names, env):
    """(the child of the tests below) the fixtures `names` under the environment `env`: {name/setting: digests}; the [cjs tally]
    lines go to stderr.  With "keys" in env: one line_keys call and one tally of the same window, for their D2H figures."""
    os.environ["CJS_DEBUG"] = "1"
    for k, v in env.items():
        if k not in ("CJS_RANGE_PASS_BLOCKS", "keys"):
            os.environ[k] = v
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = tc.bind(), support.Oracle(), {}
    for name in names:
        f = tc.stream_fixture(L, name, oracle)
        if "keys" in env:
            a = f["stream"]
            rc, keys, info, d = lk.keys_host(L, a, f["h"], f["t"], cap=int(f["nl"].size) + 1)
            rc2, groups, tinfo, d2 = tc.stream_tally(L, L.cjs_bzip2_tally, a.ctypes.data_as(rg.u8p), a.size, f["h"], f["t"], cap=16)
            assert rc == 0 and rc2 == 0
            out[name] = [int(info.n_lines), int(tinfo.n_lines), int(groups.size)]
            continue
        for cap in env.get("CJS_RANGE_PASS_BLOCKS", "0").split(","):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            out[name + "/" + cap] = _digests(L, f)
    print(json.dumps(out))


TALLY_LINE = r"\[cjs tally\] (host|device): lines \[(\d+), (\d+)\), mode lines, (\d+) of \d+ blocks touched, (\d+) bad, (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\).* H2D (\d+) D2H (\d+)"


def _run_child(names, env):
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_tally as t; t.child(%r, %r)" % (names, env)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=penv,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [(m[0],) + tuple(int(x) for x in m[1:]) for m in re.findall(TALLY_LINE, run.stderr)]
    return json.loads(run.stdout.strip().splitlines()[-1]), lines, run.stderr


def test_several_passes_give_the_one_pass_groups(L, fx):
    got, lines, _ = _run_child(["TL1"], {"CJS_RANGE_PASS_BLOCKS": "1,2"})
    here = _digests(L, fx["TL1"])
    assert got["TL1/1"] == here and got["TL1/2"] == here
    # not vacuous: per cap, in either form, the count query and the call with room over the whole stream, then one call over the
    # window; a pass held at most `cap` of the touched blocks
    assert len(lines) == 12, lines
    for i, (form, a, b, t, bad, p, bt, h2d, d2h) in enumerate(lines):
        cap = (1, 2)[i // 6]
        assert bad == 0 and p == (t + cap - 1) // cap and (p > 1 or i % 6 >= 4), (i, lines[i])


def test_several_batches_in_a_pass_give_the_same(L, fx):
    got, lines, _ = _run_child(["TL1"], {"CJS_DEC_BATCH_ELEMS": "150000"})
    assert got["TL1/0"] == _digests(L, fx["TL1"])
    assert len(lines) == 6 and all(p == 1 for _, _, _, _, _, p, _, _, _ in lines) and lines[0][6] >= 3, lines


def test_the_keys_did_not_come_down(fx):
    """TL1, whole lines, 16 groups asked for: what the tally brings down is below what line_keys brings down for the same window
    by at least 8 bytes a line (the records are 16)"""
    got, lines, err = _run_child(["TL1"], {"keys": "1"})
    n_lines, n_tally, n_groups = got["TL1"]
    keys_d2h = [int(x) for x in re.findall(r"\[cjs linekeys\] host: .* D2H (\d+)", err)]
    assert len(keys_d2h) == 1 and len(lines) == 1 and n_groups == 16 and n_tally == n_lines
    assert lines[0][8] <= keys_d2h[0] - 8 * n_lines, (lines, keys_d2h)


def test_a_damaged_block_counts_its_lines_and_serves_the_rest(L, fx):
    f = fx["TL1"]
    e, b, plain = f["entries"], f["bounds"], f["plain"]
    cum = np.concatenate([[0], np.cumsum(lc.block_counts(plain, b))])
    blk = 1
    damaged = f["stream"].copy()
    bit = e[blk][0] + 48 + 32 + 1 + 23          # the lowest bit of the block's BWT start
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    g = dict(f, stream=damaged, dev=lc.on_device(damaged))
    bad = set(range(int(cum[blk]), int(cum[blk + 1]) + 1))          # the lines the table gives the block, and the one that goes on behind it
    items = [None if k in bad else x for k, x in enumerate(tc.window_lines(plain))]
    for order in (tc.BY_COUNT, tc.BY_FIRST):
        groups, info = tc.both_forms(L, g, order=order)
        ref, rinfo = tc.tally_ref(items, order, bad=None)
        assert tc.stream_info_tuple(info) == rinfo + (4, 1, blk)
        assert [(a, c) for _, a, c in tc.groups_as_tuples(groups)] == [(a, c) for _, a, c in ref]
        assert int(groups["count"].sum()) == info.n_lines - info.n_bad_lines and info.n_bad_lines == len(bad)
    d = rg.detail(L)
    assert re.fullmatch(r"Bad block CRC \(got [0-9a-f]+ expected %x\)" % e[blk][3], d) or d == "index does not match the stream at block %d" % blk, d
    # a window in front of the block does not touch it
    groups, info = tc.both_forms(L, g, first=0, count=int(cum[blk - 1]) if blk > 1 else 50)
    assert info.n_bad_lines == 0 and info.n_bad_blocks == 0


def _three_crafted_blocks():
    """three blocks of a few hundred bytes (bzcraft: random ranks over newline and eight letters) -> (stream, the blocks' texts);
    a line runs from block 0 into block 1 and another from block 1 into block 2, and blocks 1 and 2 hold newlines"""
    import bzcraft
    import bzcraft_cases as bc
    used = (10,) + tuple(range(97, 105))
    for seed in range(64):
        rng = np.random.RandomState(7000 + seed)
        blocks = [bc.plain(used, bc.ranks(rng, len(used), 300)) for _ in range(3)]
        texts = [bzcraft.model(bzcraft.stream([b])) for b in blocks]
        if all(isinstance(x, bytes) and 200 <= len(x) <= 1000 for x in texts) and not texts[0].endswith(b"\n") and not texts[1].endswith(b"\n") \
                and b"\n" in texts[1] and b"\n" in texts[2]:
            return bzcraft.stream(blocks), texts
    raise AssertionError("no seed gives the three blocks")


def test_the_fills_and_the_patches_of_one_join_go_up_together(L):
    """the middle one of three small blocks is bad: its lines are filled with all-ones, the line that ends in block 2 is patched
    with all-ones, line 0 and the tail are patched with their keys -- against cjs_stage_keys_tally over the keys of the lines"""
    stream, texts = _three_crafted_blocks()
    plain = b"".join(texts)
    rc, h = rg.build(L, stream, 0)
    assert rc == 0, rg.detail(L)
    e = rg.entries(L, h)
    assert [x[2] for x in e] == [len(x) for x in texts]
    t = lc.build_both(L, stream, h, lc.on_device(stream))
    cum = np.concatenate([[0], np.cumsum([x.count(b"\n") for x in texts])])
    damaged = stream.copy()
    bit = e[1][0] + 48 + 32 + 1 + 23          # the lowest bit of the block's BWT start
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    g = dict(stream=damaged, dev=lc.on_device(damaged), h=h, t=t)
    seed = SEEDS[1]
    # the tally's lines: every newline's, and the tail's as if it ended in one (an empty tail is no line)
    rc, keys, n = lk.stage_keys(L, plain if plain.endswith(b"\n") else plain + b"\n", seed)
    assert rc == 0 and n == keys.size == int(cum[3]) + 1 + (not plain.endswith(b"\n"))
    keys = keys[:-1]
    bad = range(int(cum[1]), int(cum[2]) + 1)          # the lines the table gives block 1, and the one that goes on behind it
    for k in bad:
        keys[k] = tc.ONES
    for order in (tc.BY_COUNT, tc.BY_FIRST):
        groups, info = tc.both_forms(L, g, seed=seed, order=order)
        rc, ref, rinfo = tc.stage_tally(L, keys, order)
        assert rc == 0 and rinfo.n_bad == len(bad) >= 2
        assert tc.stream_info_tuple(info) == tc.info_tuple(rinfo) + (3, 1, 1)
        assert groups.tobytes() == ref.tobytes()


def test_a_window_above_the_line_limit_is_refused(L, fx):
    """the limit is 2^32 - 2 lines and no table of that many fits a test: cjs_stage_bzip2_tally_limit takes it as an argument"""
    f = fx["TL1"]
    a, N = f["stream"], int(f["nl"].size)

    def limited(form, first, count, limit):
        info = tc.StreamInfo()
        out = np.zeros(4, dtype=tc.TALLY)
        src = (a.ctypes.data, None) if form == "host" else (None, f["dev"][1])
        return L.cjs_stage_bzip2_tally_limit(src[0], src[1], a.size, f["h"], f["t"], first, count, limit, out.ctypes.data, 4, ctypes.byref(info), None), info, out
    for form in ("host", "device"):
        assert limited(form, 0, tc.M64, 100)[0] == tc.E_UNSUPPORTED
        assert limited(form, N - 200, 101, 100)[0] == tc.E_UNSUPPORTED
        rc, info, out = limited(form, N - 200, 100, 100)
        assert rc == 0 and info.n_lines == 100
        rc, info, out = limited(form, 0, tc.M64, 2 ** 40)          # (never above the sorter's own limit)
        want, winfo = tc.both_forms(L, f, cap=4)
        assert rc == 0 and info.n_lines == N + 1 and out.tobytes() == want.tobytes() and tc.stream_info_tuple(info) == tc.stream_info_tuple(winfo)
    assert L.cjs_stage_bzip2_tally_limit(a.ctypes.data, f["dev"][1], a.size, f["h"], f["t"], 0, 5, 100, None, 0, ctypes.byref(tc.StreamInfo()), None) == tc.E_INVALID


# ---- the tally of a cut: the piece keys, then the modes CJS_CUT_FIELDS / CJS_CUT_BYTES
PIECE = 1000


def text_keys(L, torch, text, seed=0, piece=PIECE, cap=None):
    """cjs_stage_text_keys_device of `text` at an odd device address -> (rc, keys as tuples, n_lines)"""
    raw = np.frombuffer(bytes(text), dtype=np.uint8)
    d = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    if raw.size:
        d[3:3 + raw.size] = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    cap = bytes(text).count(b"\n") + 1 if cap is None else cap
    buf, ptr = lk._guarded(lk.KEY, cap)
    n = rg.S(0)
    rc = L.cjs_stage_text_keys_device(d.data_ptr() + 3 if raw.size else None, raw.size, seed, ptr if cap else None, cap, ctypes.byref(n), piece, None)
    keys = lk._unguard(buf, lk.KEY, cap, min(cap, n.value) if rc == 0 else 0)
    return rc, lk.as_tuples(keys), n.value


def _texts():
    rng = np.random.RandomState(5)
    word = lambda n: bytes(rng.randint(97, 123, n).astype(np.uint8))
    P = PIECE
    return {
        "empty": b"", "one byte": b"x", "one newline": b"\n", "no newline": word(2500),
        "a newline as the last byte of a piece": word(P - 1) + b"\n" + word(40) + b"\nzz",
        "a newline as the first byte of the next piece": word(P) + b"\n" + word(40) + b"\n",
        "a newline on either side of a seam": word(P - 1) + b"\n\n" + word(P - 2) + b"\n\n\n",
        "a line over three pieces": b"ab\n" + word(2 * P + 300) + b"\ncd\n" + word(17),
        "piece size - 1": word(300) + b"\n" + word(P - 302), "piece size exact": word(300) + b"\n" + word(P - 301),
        "piece size + 1": word(300) + b"\n" + word(P - 300), "two pieces exact, ending in a newline": word(2 * P - 1) + b"\n",
        "0x00 and 0xFF bytes": bytes(rng.choice(np.array([0, 0, 255, 255, 10, 97], np.uint8), 3 * P + 7)),
        "short lines over many pieces": b"".join(word(int(k)) + b"\n" for k in rng.randint(0, 9, 2000)),
        "more than a tile to a piece": b"".join(word(int(k)) + b"\n" for k in rng.randint(0, 200, 600)),
    }


TEXTS = _texts()


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_text_keys_in_pieces_against_the_host_keys(L, torch, name):
    text = TEXTS[name]
    for seed in SEEDS:
        rc, want, n_want = lk.stage_keys(L, text, seed)
        want = lk.as_tuples(want)
        assert rc == 0 and want == lk.text_keys(text, seed) and n_want == len(want)
        pieces = (PIECE, 0) if name != "more than a tile to a piece" else (40000, 16384, 16385)          # (0: the product's 900,000)
        for piece in pieces:
            rc, got, n_got = text_keys(L, torch, text, seed, piece)
            assert rc == 0 and n_got == n_want and got == want, (name, seed, piece)
    rc, got, n_got = text_keys(L, torch, text, 0, PIECE, cap=1)          # a short array: the first record alone, the count in full
    assert rc == 0 and n_got == text.count(b"\n") + 1 and got == lk.text_keys(text, 0)[:1]


CUTS = ((tc.FIELDS, 9, [(2, 2)]), (tc.FIELDS, 9, [(1, 1), (3, 3)]), (tc.BYTES, 0, [(1, 8)]))


@pytest.mark.parametrize("name", STREAMS)
def test_the_tally_of_a_cut_against_the_cut_lines(L, fx, name):
    f = fx[name]
    N = int(f["nl"].size)
    for k, cut in enumerate(CUTS):
        mode, d, sel = cut
        for i, (first, count, order, lo, hi, cap) in enumerate(((0, None, tc.BY_COUNT, 1, 0, None), (0, None, tc.BY_FIRST, 2, 0, None), (N // 3, N // 2, tc.BY_FIRST, 1, 0, None),
                                                                (5, None, tc.BY_COUNT, 1, 1, 7), (N, None, tc.BY_COUNT, 1, 0, None))):
            if name == "CT2" and i not in (0, 2):
                continue          # (639 blocks a call)
            seed = SEEDS[(i + k) & 1]
            groups, info = tc.both_forms(L, f, first=first, count=tc.M64 if count is None else count, seed=seed, mode=mode, d=d, sel=sel, order=order, min_count=lo,
                                         max_count=hi, cap=cap)
            tc.check_against_the_lines(groups, info, f["plain"], seed, first, count, order, lo, hi, cap, cut=cut)
            assert info.n_bad_lines == 0 and info.n_bad_blocks == 0


def test_a_damaged_block_fails_the_tally_of_a_cut_as_it_fails_the_cut(L, fx):
    import cut_cases as ct
    Lc = ct.bind()                                          # (the same library, with the cut's argument types)
    f = fx["TL1"]
    e = f["entries"]
    blk = 1
    damaged = f["stream"].copy()
    bit = e[blk][0] + 48 + 32 + 1 + 23          # the lowest bit of the block's BWT start
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    dev = lc.on_device(damaged)
    for mode, d, sel in CUTS:
        rc_c, _, cinfo, cdet = ct.cut_host(Lc, damaged, f["h"], f["t"], mode, d, sel)
        assert rc_c == rg.E_DATA and cdet
        for fn, src in ((L.cjs_bzip2_tally, damaged.ctypes.data_as(rg.u8p)), (L.cjs_bzip2_tally_device, dev[1])):
            rc, groups, info, det = tc.stream_tally(L, fn, src, damaged.size, f["h"], f["t"], mode=mode, d=d, sel=sel, cap=8)
            assert rc == rc_c and det == cdet and groups.size == 0, (rc, det, cdet)
            assert (info.n_bad_blocks, info.first_bad_block, info.blocks_decoded) == (cinfo.n_bad_blocks, cinfo.first_bad_block, cinfo.blocks_decoded) == (1, blk, 4)
        # a window in front of the block is served
        rc, groups, info, det = tc.stream_tally(L, L.cjs_bzip2_tally, damaged.ctypes.data_as(rg.u8p), damaged.size, f["h"], f["t"], first=0, count=50, mode=mode, d=d,
                                                sel=sel, cap=None)
        assert rc == 0
        tc.check_against_the_lines(groups, info, f["plain"], 0, 0, 50, cut=(mode, d, sel))


def test_stream_argument_errors(L, fx):
    f, other = fx["TL1"], fx["CT2"]
    a = f["stream"]
    src = a.ctypes.data_as(rg.u8p)
    for fn, s in ((L.cjs_bzip2_tally, src), (L.cjs_bzip2_tally_device, f["dev"][1])):
        rc, _, _, d = tc.stream_tally(L, fn, s, a.size, f["h"], other["t"], cap=4)
        assert rc == tc.E_INVALID and d == lc.FOREIGN
        assert tc.stream_tally(L, fn, s, a.size, f["h"], f["t"], cap=4, order=2)[0] == tc.E_INVALID
        assert tc.stream_tally(L, fn, s, a.size, f["h"], f["t"], cap=4, min_count=3, max_count=2)[0] == tc.E_INVALID
        assert tc.stream_tally(L, fn, s, a.size, f["h"], f["t"], cap=4, mode=3)[0] == tc.E_INVALID
        for bad_sel in ([(0, 1)], [(3, 2)], [], [(k, k) for k in range(1, 66)]):          # the cut's selection errors
            assert tc.stream_tally(L, fn, s, a.size, f["h"], f["t"], cap=4, mode=tc.FIELDS, d=9, sel=bad_sel)[0] == tc.E_INVALID
        assert tc.stream_tally(L, fn, s, a.size, f["h"], f["t"], cap=4, mode=tc.FIELDS, d=10, sel=[(1, 1)])[0] == tc.E_INVALID
        assert tc.stream_tally(L, fn, s, a.size - 1, f["h"], f["t"], cap=4)[0] == tc.E_INVALID
    info = tc.StreamInfo()
    assert L.cjs_bzip2_tally(src, a.size, f["h"], f["t"], 0, 4, 0, tc.LINES, 0, None, 0, tc.BY_COUNT, 1, 0, None, 4, ctypes.byref(info), None) == tc.E_INVALID
    assert L.cjs_bzip2_tally(src, a.size, f["h"], f["t"], 0, 4, 0, tc.LINES, 0, None, 0, tc.BY_COUNT, 1, 0, None, 0, None, None) == tc.E_INVALID
