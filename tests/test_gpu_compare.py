"""Compare on the GPU (cjs_bzip2_compare[_device], cjs_bzip2_compare_streams[_device], Bzip2Index.compare / compare_stream): every
list against numpy.nonzero(plain != other) on the decoded text -- at every alignment of the two sides, across block, tile and
window seams, passes and batches, clipped windows, caps, blocks of a few bytes, damaged blocks on either side and two streams
whose blocks fall differently.  Every case runs the host form and the device form (compare_cases.both_forms)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import compare_cases as cc
import range_cases as rg
import search_cases as sc

pytestmark = pytest.mark.gpu

NONE = cc.NONE


@pytest.fixture(scope="module")
def L():
    return cc.bind()


def _indexed(L, stream, multi):
    rc, h = rg.build(L, stream, multi)
    assert rc == 0, (rc, rg.detail(L))
    e = rg.entries(L, h)
    bounds = np.concatenate([[0], np.cumsum([x[2] for x in e])]).astype(np.int64)
    return h, e, bounds


def _fixture(L, name, oracle):
    if name in ("F1", "F2"):
        stream, plain, multi, _ = rg.fixture(name, oracle)
    else:
        stream, plain, multi = sc.s4(oracle)
    h, e, bounds = _indexed(L, stream, multi)
    return dict(stream=stream, plain=plain, h=h, entries=e, bounds=bounds, total=int(bounds[-1]), multi=multi)


@pytest.fixture(scope="module")
def fx(L, oracle):
    return {name: _fixture(L, name, oracle) for name in ("F1", "F2", "S4")}


def _blocks_of(f, lo, hi):
    """blocks of non-zero size that [lo, hi) overlaps"""
    b = f["bounds"]
    return sum(1 for k in range(len(b) - 1) if b[k + 1] > b[k] and b[k] < hi and b[k + 1] > lo) if lo < hi else 0


def _info(want, compared, blocks, bad=(0, NONE), bad_b=(0, NONE)):
    return (len(want), want[0][0] if want else NONE, compared, bad[0], bad[1], blocks, bad_b[0], bad_b[1])


def _sweep_flips(f):
    """the flip set of the alignment sweep (cc.seam_flips), and the tile seams as they fall behind a window start of 0..15"""
    pos = set(cc.seam_flips(f["bounds"]))
    pos |= {s + 16384 * k + d for s in range(16) for k in (1, 2) for d in (-1, 0, 1)}
    return cc.flipped(f["plain"], pos, seed=3)


@pytest.mark.parametrize("name", ["F1", "F2", "S4"])
def test_equal(L, fx, name):
    f = fx[name]
    got, info, d = cc.both_forms(L, f["stream"], f["h"], f["plain"])
    assert got == [] and d == ""
    assert info == (0, NONE, f["total"], 0, NONE, _blocks_of(f, 0, f["total"]), 0, NONE)


def test_every_alignment_of_the_other_side(L, fx):
    f = fx["F1"]
    other = _sweep_flips(f)
    want, compared = cc.expected(f["plain"], other)
    b = f["bounds"]
    assert len(want) > 100 and compared == f["total"] and want[0][0] == 0 and want[-1][0] == f["total"] - 1
    assert {int(b[5]) + d for d in range(-7, 8)} <= {o for o, x, y in want}
    for r in range(16):
        got, info, d = cc.both_forms(L, f["stream"], f["h"], other, shift_other=r, shift_in=(5 * r + 1) % 16)
        assert got == want and info == _info(want, compared, 10) and d == "", r


def test_every_window_start_and_end(L, fx):
    f = fx["F1"]
    other = _sweep_flips(f)
    B5 = int(f["bounds"][5])
    for s in range(16):                                     # the segment of block 0 starts at s: its tile seams move with it
        want, compared = cc.expected(f["plain"], other, off=s)
        got, info, d = cc.both_forms(L, f["stream"], f["h"], other, off=s, shift_other=(3 * s + 2) % 16)
        assert got == want and info == _info(want, compared, 10) and compared == f["total"] - s, s
    for e in range(16):                                     # ends inside the 15 flipped bytes across the seam of blocks 4 and 5
        end = B5 - 7 + e
        want, compared = cc.expected(f["plain"], other, off=7, ln=end - 7)
        got, info, d = cc.both_forms(L, f["stream"], f["h"], other, off=7, ln=end - 7, shift_other=e)
        assert got == want and info == _info(want, compared, _blocks_of(f, 7, end)) and compared == end - 7, e
        assert (want[-1][0] == end - 1) == (e >= 1)


def test_clipping(L, fx):
    f = fx["F1"]
    plain, total, b = f["plain"], f["total"], f["bounds"]
    flipped = cc.flipped(plain, cc.random_flips(total, 3000, 11) + cc.seam_flips(b), seed=4)
    longer = np.concatenate([flipped, np.arange(100, dtype=np.uint8)])
    lo37, hi37 = int(b[3]) + 1234, int(b[7]) + 777
    cases = [
        # (other, other_off, off, ln)
        (flipped[:500000], 0, 0, cc.ALL),                                    # the other side shorter
        (longer, 0, 0, cc.ALL),                                              # longer
        (flipped[lo37:hi37], lo37, 0, cc.ALL),                               # starts inside block 3, ends inside block 7
        (flipped[lo37:hi37], lo37, int(b[4]) - 3, int(b[6] - b[4]) + 5),     # a window inside it
        (flipped[lo37:hi37], lo37, int(b[2]), hi37),                         # a window that hangs over on both sides
        (flipped[5000:5100], 5000, 4000, 1001),                              # an overlap of one byte ...
        (cc.flipped(plain, [5000])[5000:5100], 5000, 4000, 1001),            # ... that differs
        (flipped[5000:5001], 5000, 0, cc.ALL),                               # another
        (flipped[int(b[9]):], int(b[9]), int(b[8]) + 5, cc.ALL),             # off + len wraps: to the end
        (flipped, 0, int(b[8]) + 5, 2 ** 64 - 4),
        (flipped, 0, 2 ** 63, 2 ** 63 + 100),
    ]
    for k, (other, o_off, off, ln) in enumerate(cases):
        span_lo, span_hi = max(off, o_off), min(off + ln, total, o_off + other.size)
        want, compared = cc.expected(plain, other, o_off, off, ln)
        assert compared == max(span_hi - span_lo, 0)
        got, info, d = cc.both_forms(L, f["stream"], f["h"], other, o_off, off, ln, shift_other=(7 * k) % 16)
        assert got == want and info == _info(want, compared, _blocks_of(f, span_lo, span_hi)) and d == "", k
        assert all(span_lo <= o < span_hi for o, x, y in got)
    assert [cc.expected(plain, c[0], c[1], c[2], c[3])[1] for c in cases[5:8]] == [1, 1, 1] and len(cc.expected(plain, *cases[6])[0]) == 1
    # no overlap at all: zeros, nothing decoded
    for other, o_off, off, ln in ((flipped[:5000], 0, 5000, cc.ALL), (flipped[5000:6000], 5000, 0, 5000), (flipped[:0], 77, 0, cc.ALL)):
        got, info, d = cc.both_forms(L, f["stream"], f["h"], other, o_off, off, ln)
        assert got == [] and info == cc.ZERO_INFO


def test_caps(L, fx):
    f = fx["F1"]
    other = cc.flipped(f["plain"], cc.random_flips(f["total"], 400, 21), seed=5)
    want, compared = cc.expected(f["plain"], other)
    n = len(want)
    assert 300 < n <= 400
    for cap in (0, 1, n - 1, n, n + 5):                     # (the canary behind record min(cap, n) is checked in compare_cases._call)
        got, info, d = cc.both_forms(L, f["stream"], f["h"], other, cap=cap)
        assert got == want[:cap] and info == _info(want, compared, 10), cap


def test_dense_block(L, fx):
    """every byte of block 4 differs: as many records as the block has bytes, contiguous, a and b bytewise"""
    f = fx["F1"]
    lo, hi = int(f["bounds"][4]), int(f["bounds"][5])
    other = f["plain"].copy()
    other[lo:hi] ^= 0xFF
    got, info, d = cc.both_forms(L, f["stream"], f["h"], other, shift_other=11)
    assert info[0] == hi - lo == len(got) and info[1] == lo
    assert [o for o, a, b in got] == list(range(lo, hi))
    assert bytes(a for o, a, b in got) == f["plain"][lo:hi].tobytes() and bytes(b for o, a, b in got) == other[lo:hi].tobytes()
    assert got == cc.expected(f["plain"], other)[0]


def _tiny_flips(f):
    """the first and last byte of every block, every byte of the blocks of at most 3 bytes"""
    b, pos = f["bounds"], set()
    for lo, hi in zip(b[:-1], b[1:]):
        if hi > lo:
            pos |= {int(lo), int(hi) - 1} | (set(range(int(lo), int(hi))) if hi - lo <= 3 else set())
    return sorted(pos)


@pytest.mark.parametrize("name", ["S4", "F2"])
def test_tiny_blocks(L, fx, name):
    f = fx[name]
    e, b = f["entries"], f["bounds"]
    # not vacuous: blocks of one byte (S4), and blocks whose last byte stands in front of a member without a block (a gap of two
    # stream headers and trailers between the blocks)
    before_empty = [int(b[k + 1]) - 1 for k in range(len(e) - 1) if e[k][2] and e[k + 1][0] - e[k][1] > 200]
    assert len(before_empty) >= 3 and (name != "S4" or sum(1 for x in e if x[2] == 1) >= 5)
    flips = _tiny_flips(f)
    assert set(before_empty) <= set(flips)
    other = cc.flipped(f["plain"], flips, seed=6)
    want, compared = cc.expected(f["plain"], other)
    assert [o for o, x, y in want] == flips
    got, info, d = cc.both_forms(L, f["stream"], f["h"], other, shift_other=13)
    assert got == want and info == _info(want, compared, _blocks_of(f, 0, f["total"])) and d == ""
    got, info, d = cc.both_forms(L, f["stream"], f["h"], other[1:-1], other_off=1, off=2, cap=5)
    want, compared = cc.expected(f["plain"], other[1:-1], 1, 2)
    assert got == want[:5] and info[:3] == (len(want), want[0][0], f["total"] - 3)


# ---- passes, batches and windows: child processes (the settings are read per call, CJS_DEBUG once per process)
def _split_cases(fx):
    sets = {"F1": _sweep_flips, "S4": lambda f: cc.flipped(f["plain"], _tiny_flips(f), seed=6)}
    return {name: (fx[name], sets[name](fx[name])) for name in ("F1", "S4") if name in fx}


def child(names, env):
    """(the child of the tests below) the fixtures `names` under the environment `env`: {name/setting: result of both_forms};
    the [cjs compare] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    for k, v in env.items():
        if k != "CJS_RANGE_PASS_BLOCKS":
            os.environ[k] = v
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = cc.bind(), support.Oracle(), {}
    fx = {name: _fixture(L, name, oracle) for name in names}
    for name in names:
        f, other = _split_cases(fx)[name]
        for cap in env.get("CJS_RANGE_PASS_BLOCKS", "0").split(","):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            got, info, d = cc.both_forms(L, f["stream"], f["h"], other)
            out[name + "/" + cap] = [got, list(info), d]
    print(json.dumps(out))


def child_streams(env):
    """(a child as well) F1 against its level-9 twin with 100 flips, under `env`"""
    os.environ["CJS_DEBUG"] = "1"
    os.environ.update(env)
    import torch  # noqa: F401
    import support
    L, oracle = cc.bind(), support.Oracle()
    f = _fixture(L, "F1", oracle)
    t = _twin(L, oracle, cc.flipped(f["plain"], _twin_flips(f), seed=7), 9)
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], t["stream"], t["h"])
    print(json.dumps([got, list(info), d]))


LINE = re.compile(r"\[cjs compare\] (host|device)( streams)?: window \[\d+, \d+\), (\d+) of \d+ blocks touched, \d+ bad, (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\), "
                  r"(\d+) windows.*?other side uploaded (\d+) B, H2D (\d+) D2H (\d+) \(of these the compare's own: H2D (\d+) D2H (\d+)\), (\d+) diffs, (\d+) compared")


def _run_child(call):
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", "import test_gpu_compare as t; t." + call], capture_output=True, text=True, env=penv,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    keys = ("form", "streams", "touched", "passes", "batches", "windows", "other_up", "h2d", "d2h", "own_h2d", "own_d2h", "diffs", "compared")
    lines = [dict(zip(keys, [m[0], bool(m[1])] + [int(x) for x in m[2:]])) for m in LINE.findall(run.stderr)]
    return json.loads(run.stdout.strip().splitlines()[-1]), lines


def _as_json(res):
    got, info, d = res
    return [[list(m) for m in got], list(info), d]


def test_several_passes_give_the_one_pass_list(L, fx):
    got, lines = _run_child("child(%r, %r)" % (["F1", "S4"], {"CJS_RANGE_PASS_BLOCKS": "1,3"}))
    for name, (f, other) in _split_cases(fx).items():
        here = cc.both_forms(L, f["stream"], f["h"], other)
        assert here[0] == cc.expected(f["plain"], other)[0]
        for cap in ("1", "3"):
            assert got[name + "/" + cap] == _as_json(here), (name, cap)
    # not vacuous: a pass held at most 1 (then 3) of the touched blocks
    assert len(lines) == 16 and all(x["passes"] >= 4 for x in lines), lines
    assert any(x["passes"] == x["touched"] for x in lines) and any(x["passes"] == (x["touched"] + 2) // 3 for x in lines)


def test_several_batches_in_a_pass_give_the_same(L, fx):
    """F1 with at most 250,000 BWT bytes to an inverse-BWT batch (two blocks)"""
    got, lines = _run_child("child(%r, %r)" % (["F1"], {"CJS_DEC_BATCH_ELEMS": "250000"}))
    f, other = _split_cases(fx)["F1"]
    assert got["F1/0"] == _as_json(cc.both_forms(L, f["stream"], f["h"], other))
    assert len(lines) == 4 and all(x["passes"] == 1 and x["batches"] >= 4 for x in lines), lines


def _cap_cases(f):
    """S4 against: a flip at both ends of every block (differences in every batch), and flips in its first three bytes only"""
    everywhere, front = cc.flipped(f["plain"], _tiny_flips(f), seed=6), cc.flipped(f["plain"], [0, 1, 2], seed=8)
    n = len(cc.expected(f["plain"], everywhere)[0])
    return [(everywhere, n // 2), (everywhere, 1), (front, 2), (front, 3)]


def child_caps(elems):
    """(a child as well) S4 with at most `elems` BWT bytes to an inverse-BWT batch: [result of both_forms(other, cap=cap)] for
    every case of _cap_cases; the [cjs compare] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    os.environ["CJS_DEC_BATCH_ELEMS"] = elems
    import torch  # noqa: F401
    import support
    L = cc.bind()
    f = _fixture(L, "S4", support.Oracle())
    print(json.dumps([list(cc.both_forms(L, f["stream"], f["h"], other, cap=cap)) for other, cap in _cap_cases(f)]))


def test_cap_runs_out_in_a_later_batch(L, fx):
    """S4 in inverse-BWT batches of at most 40 bytes (its 234 bytes, at least 195 after RLE1: five batches or more in one pass).
    The list gets full in the middle of a later batch, in the first batch with differences in every later one, and in the first
    batch with none behind it: the first cap differences, and n_diffs, first_diff and compared count on."""
    f = fx["S4"]
    cases = _cap_cases(f)
    want = cc.expected(f["plain"], cases[0][0])[0]
    assert len(want) > 100 and want[len(want) // 2][0] > 80 and want[-1][0] == f["total"] - 1
    got, lines = _run_child("child_caps('40')")
    for (other, cap), res in zip(cases, got):
        want, compared = cc.expected(f["plain"], other)
        assert res == _as_json((want[:cap], _info(want, compared, _blocks_of(f, 0, f["total"])), "")), cap
    assert len(lines) == 4 * len(cases) and all(x["passes"] == 1 and x["batches"] >= 5 for x in lines), lines


def test_device_form_moves_no_bulk(L, fx):
    """From the [cjs compare] lines of a default run of F1 (938,848 decoded bytes, 10 blocks).  The compare's own traffic per
    batch is 16 bytes to the host (the batch's count and first offset) and one 40-byte segment per run of good blocks to the
    device; the records delivered are 16 bytes each.  The engine's own traffic is per block and per pass (candidates, block
    headers, row and batch tables, slice lists: a few hundred bytes per block), which 1 KiB per touched block + 4 KiB per pass
    bounds with room; nothing in either direction grows with the decoded size."""
    got, lines = _run_child("child(%r, %r)" % (["F1"], {}))
    f, other = _split_cases(fx)["F1"]
    n = len(cc.expected(f["plain"], other)[0])
    assert len(lines) == 4 and [x["form"] for x in lines] == ["host", "host", "device", "device"]
    for x, cap in zip(lines, (0, n, 0, n)):
        assert x["diffs"] == n and x["compared"] == f["total"]
        engine = 1024 * x["touched"] + 4096 * x["passes"]
        assert x["own_d2h"] <= 16 * min(cap, n) + 16 * x["batches"], x
        assert x["d2h"] <= x["own_d2h"] + engine, x
        if x["form"] == "device":
            assert x["other_up"] == 0 and x["own_h2d"] <= 40 * x["touched"] and x["h2d"] <= x["own_h2d"] + engine, x
        else:                                               # the host form uploads the stream's block bytes and the other side once
            assert x["other_up"] == f["total"] and x["own_h2d"] <= x["other_up"] + 40 * x["touched"], x


# ---- damage
def _flip_payload_bit(stream, e):
    pos = (e[0] + e[1]) // 2
    rg.set_bits(stream, pos, 1, 1 - rg.bits(stream, pos, 1))


def _read_ranges_detail(L, stream, h, lo, hi):
    rc, buf, off, ln, st, d = rg.read_host(L, stream, h, [(lo, hi - lo)])
    assert rc == 0 and st[0] == rg.E_DATA
    return d


def test_damage(L, fx):
    f = fx["F1"]
    e, b, plain, total = f["entries"], [int(x) for x in f["bounds"]], f["plain"], f["total"]
    other = cc.flipped(plain, cc.seam_flips(b) + cc.random_flips(total, 200, 31), seed=8)
    # one payload bit of block 5
    damaged = f["stream"].copy()
    _flip_payload_bit(damaged, e[5])
    want, compared = cc.expected(plain, other, runs=[(0, b[5]), (b[6], total)])
    got, info, d = cc.both_forms(L, damaged, f["h"], other)
    assert got == want and info == _info(want, total - e[5][2], 10, bad=(1, 5)) and compared == total - e[5][2]
    assert d == _read_ranges_detail(L, damaged, f["h"], b[5], b[6]) and d != ""
    assert any(o < b[5] for o, x, y in got) and any(o >= b[6] for o, x, y in got) and not any(b[5] <= o < b[6] for o, x, y in got)
    # blocks 0 and 9: the magic of one, a payload bit of the other
    damaged = f["stream"].copy()
    rg.set_bits(damaged, e[0][0], 48, 0x314159265358)
    _flip_payload_bit(damaged, e[9])
    want, compared = cc.expected(plain, other, runs=[(b[1], b[9])])
    got, info, d = cc.both_forms(L, damaged, f["h"], other)
    assert got == want and info == _info(want, b[9] - b[1], 10, bad=(2, 0)) and d == "index does not match the stream at block 0"
    got, info, d = cc.both_forms(L, damaged, f["h"], other, off=b[8] + 100)      # block 9 is the first bad one of this window
    want, compared = cc.expected(plain, other, off=b[8] + 100, runs=[(b[1], b[9])])
    assert got == want and info == _info(want, b[9] - b[8] - 100, 2, bad=(1, 9)) and d == _read_ranges_detail(L, damaged, f["h"], b[9], total)
    # an index entry that does not match the stream: the CRC of block 3
    rows = [list(x) for x in e]
    rows[3][3] ^= 0x10
    rc, h2 = rg.create(L, rows, f["stream"].size, 0)
    assert rc == 0
    want, compared = cc.expected(plain, other, runs=[(0, b[3]), (b[4], total)])
    got, info, d = cc.both_forms(L, f["stream"], h2, other)
    assert got == want and info == _info(want, total - e[3][2], 10, bad=(1, 3)) and d == "index does not match the stream at block 3"
    L.cjs_bzip2_index_destroy(h2)


# ---- two streams
def _twin(L, oracle, plain, level):
    rc, s = oracle.bzip2_compress(plain, level)
    assert rc == 0
    stream = np.asarray(s, dtype=np.uint8)
    h, e, bounds = _indexed(L, stream, 0)
    return dict(stream=stream, plain=plain, h=h, entries=e, bounds=bounds, total=int(bounds[-1]))


def _twin_flips(f):
    return cc.random_flips(f["total"], 100, 41) + [0, f["total"] - 1, 99999, 100000, 899999, 900000]


def test_two_streams_equal_and_flipped(L, fx, oracle):
    f = fx["F1"]
    t9 = _twin(L, oracle, f["plain"], 9)
    assert len(t9["entries"]) == 2 and len(f["entries"]) == 10      # the block boundaries differ
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], t9["stream"], t9["h"])
    assert got == [] and info == (0, NONE, f["total"], 0, NONE, 10, 0, NONE) and d == ""
    got, info, d = cc.both_forms_streams(L, t9["stream"], t9["h"], f["stream"], f["h"], shift_a=0, shift_b=15)      # the other way round
    assert got == [] and info == (0, NONE, f["total"], 0, NONE, 2, 0, NONE)
    other = cc.flipped(f["plain"], _twin_flips(f), seed=7)
    tf = _twin(L, oracle, other, 9)
    want, compared = cc.expected(f["plain"], other)
    assert 100 <= len(want) <= 106
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], tf["stream"], tf["h"])
    assert got == want and info == _info(want, f["total"], 10)
    for cap in (0, 1, len(want) - 1, len(want) + 5):
        got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], tf["stream"], tf["h"], cap=cap)
        assert got == want[:cap] and info == _info(want, f["total"], 10)
    lo, ln = int(f["bounds"][2]) + 17, 300000                                    # a window
    want, compared = cc.expected(f["plain"], other, off=lo, ln=ln)
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], tf["stream"], tf["h"], off=lo, ln=ln)
    assert got == want and info == _info(want, ln, _blocks_of(f, lo, lo + ln))
    for t in (t9, tf):
        L.cjs_bzip2_index_destroy(t["h"])


def test_two_streams_of_unequal_length(L, fx, oracle):
    import importlib
    pkg = importlib.import_module("compressjs-flattened_amd")
    f = fx["F1"]
    plain, total = f["plain"], f["total"]
    ix = pkg.Bzip2Index.build(f["stream"])
    for other, text in ((plain[:-1], "EOF on b"), (plain[:int(f["bounds"][9])], "EOF on b"), (np.concatenate([plain, [65]]).astype(np.uint8), "EOF on a")):
        t = _twin(L, oracle, other, 9)
        got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], t["stream"], t["h"])
        n = min(total, other.size)
        assert got == [] and info == (0, NONE, n, 0, NONE, _blocks_of(f, 0, n), 0, NONE)
        res = ix.compare_stream(f["stream"], t["stream"], pkg.Bzip2Index.build(t["stream"]))
        assert res.cmp_text() == text and not res.equal and (res.len_a, res.len_b, res.compared) == (total, other.size, n)
        L.cjs_bzip2_index_destroy(t["h"])
    other = cc.flipped(plain, [total - 2])[:-1]                                  # a difference in front of the end: cmp names it
    t = _twin(L, oracle, other, 9)
    res = ix.compare_stream(f["stream"], t["stream"], pkg.Bzip2Index.build(t["stream"]))
    assert res.cmp_text() == "differ: byte %d" % (total - 1) and res.diffs == [(total - 2, int(plain[total - 2]), int(other[total - 2]))]
    L.cjs_bzip2_index_destroy(t["h"])


def test_several_windows_give_the_one_window_list(L, fx, oracle):
    """windows of 100,000 decoded bytes: 10 of them, their edges inside the blocks of A (99,981 bytes each) and of B (900,000)"""
    got, lines = _run_child("child_streams(%r)" % ({"CJS_COMPARE_WINDOW_BYTES": "100000"},))
    f = fx["F1"]
    assert all(int(b) % 100000 for b in f["bounds"][1:-1])
    other = cc.flipped(f["plain"], _twin_flips(f), seed=7)
    t = _twin(L, oracle, other, 9)
    here = cc.both_forms_streams(L, f["stream"], f["h"], t["stream"], t["h"])
    assert here[0] == cc.expected(f["plain"], other)[0] and got == _as_json(here)
    assert len(lines) == 4 and all(x["streams"] and x["windows"] == 10 for x in lines), lines
    L.cjs_bzip2_index_destroy(t["h"])


def test_two_streams_damage_in_b(L, fx, oracle):
    f = fx["F1"]
    plain, total = f["plain"], f["total"]
    other = cc.flipped(plain, _twin_flips(f) + cc.random_flips(total, 200, 43), seed=9)
    t = _twin(L, oracle, other, 3)
    assert len(t["entries"]) == 4
    tb = [int(x) for x in t["bounds"]]
    damaged = t["stream"].copy()
    _flip_payload_bit(damaged, t["entries"][1])
    want, compared = cc.expected(plain, other, runs=[(0, tb[1]), (tb[2], total)])
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], damaged, t["h"])
    assert got == want and info == _info(want, total - (tb[2] - tb[1]), 10, bad_b=(1, 1)) and compared == info[2]
    assert d == _read_ranges_detail(L, damaged, t["h"], tb[1], tb[2])
    # damage on both sides: A's block 8 and B's block 1; the detail is A's
    dam_a = f["stream"].copy()
    rg.set_bits(dam_a, f["entries"][8][0], 48, 0x314159265358)
    b = [int(x) for x in f["bounds"]]
    want, compared = cc.expected(plain, other, runs=[(0, tb[1]), (tb[2], b[8]), (b[9], total)])
    got, info, d = cc.both_forms_streams(L, dam_a, f["h"], damaged, t["h"])
    assert got == want and info == _info(want, compared, 10, bad=(1, 8), bad_b=(1, 1)) and d == "index does not match the stream at block 8"
    L.cjs_bzip2_index_destroy(t["h"])


def test_many_members_against_one(L, fx, oracle):
    f = fx["F2"]
    t = _twin(L, oracle, f["plain"], 9)
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], t["stream"], t["h"])
    assert got == [] and info == (0, NONE, f["total"], 0, NONE, _blocks_of(f, 0, f["total"]), 0, NONE)
    got, info, d = cc.both_forms_streams(L, t["stream"], t["h"], f["stream"], f["h"])
    assert got == [] and info == (0, NONE, f["total"], 0, NONE, 1, 0, NONE)
    other = cc.flipped(f["plain"], _tiny_flips(f), seed=10)
    t2 = _twin(L, oracle, other, 9)
    want, compared = cc.expected(f["plain"], other)
    got, info, d = cc.both_forms_streams(L, f["stream"], f["h"], t2["stream"], t2["h"])
    assert got == want and info[:3] == (len(want), want[0][0], f["total"])
    for x in (t, t2):
        L.cjs_bzip2_index_destroy(x["h"])


def test_python_front(fx, oracle):
    import importlib
    import torch
    pkg = importlib.import_module("compressjs-flattened_amd")
    f = fx["F1"]
    stream, plain, total = f["stream"], f["plain"], f["total"]
    ix = pkg.Bzip2Index.build(stream)
    res = ix.compare(stream, plain)
    assert res.equal and res.cmp_text() == "" and (res.diffs, res.total, res.first_diff, res.compared, res.len_a, res.len_b) == ([], 0, None, total, total, total)
    assert (res.bad_blocks, res.first_bad_block, res.bad_blocks_b, res.first_bad_block_b, res.detail) == (0, None, 0, None, "")
    other = cc.flipped(plain, cc.random_flips(total, 150, 51) + [400000], seed=12)
    want, compared = cc.expected(plain, other)
    res = ix.compare(stream, other)                         # the default limit: 64
    assert res.diffs == want[:64] and res.total == len(want) > 64 and res.first_diff == want[0][0] and not res.equal
    assert ix.compare(stream, other, limit=None).diffs == want
    assert ix.compare(stream, other.tobytes(), limit=0).diffs == []
    win = ix.compare(stream, other[300000:700000], off=350000, length=100000, other_off=300000, limit=None)
    assert (win.diffs, win.compared) == cc.expected(plain, other[300000:700000], 300000, 350000, 100000) and win.len_b == 700000 and not win.equal
    # cmp's line: one line_numbers question for the first difference
    lines = pkg.Bzip2Lines.build(stream, ix)
    first = want[0][0]
    assert res.cmp_text() == "differ: byte %d" % (first + 1)
    assert res.cmp_text(ix, stream, lines) == "differ: byte %d, line %d" % (first + 1, plain[:first].tobytes().count(b"\n") + 1)
    late = ix.compare(stream, cc.flipped(plain, [400000]))
    assert late.cmp_text(ix, stream, lines) == "differ: byte 400001, line %d" % (plain[:400000].tobytes().count(b"\n") + 1) and late.diffs[0][0] == 400000
    assert ix.compare(stream, plain[:-5]).cmp_text() == "EOF on b" and ix.compare(stream, np.concatenate([plain, plain[:3]])).cmp_text() == "EOF on a"
    # the device forms
    d_in, d_other = torch.from_numpy(stream).cuda(), torch.from_numpy(other).cuda()
    torch.cuda.synchronize()
    dev = pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_other.data_ptr(), other.size, limit=None)
    assert dev.diffs == want and dev.total == len(want) and dev.compared == total
    dev = pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_other.data_ptr() + 300000, 400000, off=350000, length=100000, other_off=300000, limit=None)
    assert dev.diffs == win.diffs
    rc, s9 = oracle.bzip2_compress(other, 9)
    assert rc == 0
    s9 = np.asarray(s9, dtype=np.uint8)
    ix9 = pkg.Bzip2Index.build(s9)
    two = ix.compare_stream(stream, s9, ix9, limit=None)
    assert two.diffs == want and not two.equal and ix9.compare_stream(s9, s9, ix9).equal
    d_b = torch.from_numpy(s9).cuda()
    torch.cuda.synchronize()
    two = pkg.compare_streams_device(d_in.data_ptr(), stream.size, ix, d_b.data_ptr(), s9.size, ix9, limit=10)
    assert two.diffs == want[:10] and two.total == len(want)
    with pytest.raises(pkg.CjsError):                       # host memory where the GPU's is asked for
        pkg.compare_device(d_in.data_ptr(), stream.size, ix, other.ctypes.data, other.size)
    # a damaged block
    damaged = stream.copy()
    damaged[(f["entries"][5][0] + f["entries"][5][1]) // 16] ^= 0x04
    res = ix.compare(damaged, plain)
    assert res.bad_blocks == 1 and res.first_bad_block == 5 and "block" in res.detail.lower() and not res.equal and res.compared == total - f["entries"][5][2]
    with pytest.raises(pkg.CjsError):
        res.cmp_text()
