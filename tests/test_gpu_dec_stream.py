"""Streaming Bzip2 decoder on the GPU box: cjs_bzip2_dec_* through the Python front.  Every comparison is with a golden, with the
oracle, or with the one-shot cjs_bzip2_decompress on the same bytes (code, detail and bytes)."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import bzblocks as bz
import recipes
import support

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_OUT = 1                       # out_bytes below one block's largest expansion: raised to it (52 x 100000 x L)


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    return importlib.import_module("compressjs-flattened_amd")


def _splits(n, seed, max_piece):
    """write sizes of a fixed seed: many small, some large, some empty"""
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        k = int(rng.integers(0, 4))
        piece = 0 if k == 0 else int(rng.integers(1, max(2, max_piece >> (4 * (k - 1)))))
        piece = min(piece, left)
        out.append(piece)
        left -= piece
    return out or [0]


class _Env:
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def decode(pkg, stream, multi=0, chunk=65536, out_bytes=MIN_OUT, writes=None, read_max=70001, eager=False, debug=False, track=None):
    """The whole stream through a decoder: `writes` = write sizes (default: one write), draining after each write with reads of at
    most read_max bytes, then finish and drain.  Asserts the progress contract on every iteration: after a write that took fewer
    bytes than it was given and a drain, the next write takes at least one.  Returns (code, detail, bytes read); track(dec) is
    called after every read."""
    stream = support.as_u8(stream)
    L = pkg.load_library()
    parts = []
    env = {}
    if eager:
        env["CJS_DEC_STREAM_EAGER"] = "1"
    if debug:
        env["CJS_DEBUG"] = "1"
    with _Env(**env):
        dec = pkg.Bzip2Decoder(bool(multi), chunk, out_bytes)

    def drain():
        while True:
            p = dec.read(read_max)
            assert p.size <= read_max
            if track:
                track(dec)
            if not p.size:
                break
            parts.append(p.copy())

    def result(code, detail):
        return code, detail, (np.concatenate(parts) if parts else np.empty(0, np.uint8))

    try:
        with dec:
            pos = 0
            for w in (writes if writes is not None else [stream.size]):
                piece = stream[pos: pos + w]
                pos += w
                after_short = False
                while True:
                    took = dec.write(piece)
                    assert took <= piece.size
                    assert not (after_short and piece.size) or took >= 1, "a drained decoder took nothing"
                    piece = piece[took:]
                    drain()
                    if not piece.size:
                        break
                    after_short = True
            assert pos == stream.size
            dec.finish()
            drain()
            assert dec.done and dec.read(16).size == 0
    except pkg.CjsError as e:
        return result(e.errorCode, L.cjs_last_error_detail().decode())
    return result(0, "")


def one_shot(hip, stream, multi=0):
    rc, got = hip.bzip2_decompress(stream, multi)
    return rc, (hip.last_error_detail() if rc else ""), got


def same_as_one_shot(pkg, hip, oracle, stream, multi, **kw):
    """code and detail of the one-shot call, the oracle's code; on success the one-shot bytes.  Returns (code, detail, bytes)."""
    rc1, detail1, want = one_shot(hip, stream, multi)
    rc, detail, got = decode(pkg, stream, multi, **kw)
    orc, _ = oracle.bzip2_decompress(stream, multi)
    assert (rc, detail) == (rc1, detail1) and rc == orc, (rc, detail, rc1, detail1, orc)
    if rc == 0:
        assert got.size == want.size and np.array_equal(got, want)
    return rc, detail, got


# ---------------------------------------------------------------------------------------------- goldens
def _small_cases():
    g = support.load_golden("golden_small.json")
    return [c for c in g["cases"] if c["algo"] == "Bzip2"]


@pytest.fixture(scope="module")
def small_streams(pkg):
    cases = _small_cases()
    datas = [recipes.build(c["recipe"]) for c in cases]
    out = {}
    by_level = {}
    for c, d in zip(cases, datas):
        by_level.setdefault(c["level"], []).append((c, d))
    for level, items in by_level.items():
        streams = pkg.Bzip2.compressFiles([d for _, d in items], level)
        for (c, d), s in zip(items, streams):
            assert s.size == c["out_len"] and support.sha256(s) == c["out_sha256"]
            out[(c["name"], c["level"])] = (np.array(s), d)
    return out


def test_small_goldens_count():
    assert len(_small_cases()) == 64


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: "%s-%d" % (c["name"], c["level"]))
def test_small_goldens_in_uneven_writes(pkg, small_streams, case):
    stream, data = small_streams[(case["name"], case["level"])]
    seed = int(hashlib.sha256(("%s-%d" % (case["name"], case["level"])).encode()).hexdigest()[:8], 16)
    rc, detail, got = decode(pkg, stream, 0, 65536, MIN_OUT, _splits(stream.size, seed, 200000), 70001)
    assert rc == 0 and got.size == data.size and np.array_equal(got, data)


@pytest.mark.parametrize("k", range(5))
def test_sample_streams_against_their_ref(pkg, k):
    stream = np.fromfile(os.path.join(recipes.DATA, "sample%d.bz2" % k), dtype=np.uint8)
    want = np.fromfile(os.path.join(recipes.DATA, "sample%d.ref" % k), dtype=np.uint8)
    rc, detail, got = decode(pkg, stream, 0, 65536, MIN_OUT, _splits(stream.size, 70 + k, 100000), 70001)
    assert rc == 0 and np.array_equal(got, want)


@pytest.fixture(scope="module")
def text25():
    return recipes.textgen(2500000, 21)


@pytest.mark.parametrize("level", list(range(1, 10)))
def test_every_level(pkg, oracle, text25, level):
    rc, stream = oracle.bzip2_compress(text25, level)
    assert rc == 0
    rc, detail, got = decode(pkg, stream, 0, 65536, MIN_OUT, _splits(stream.size, level, 300000), 99991)
    assert rc == 0 and np.array_equal(got, text25)


# ---------------------------------------------------------------------------------------------- edges, eager steps
@pytest.fixture(scope="module")
def two_blocks(oracle):
    data = recipes.textgen(150000, 51)
    rc, stream = oracle.bzip2_compress(data, 1)
    assert rc == 0
    rc, table = oracle.bzip2_table(stream)
    assert rc == 0 and len(table) == 2
    return data, stream, table


@pytest.mark.parametrize("multi", [0, 1])
def test_edges_empty_one_byte_and_trailing_garbage(pkg, hip, oracle, multi):
    empty = oracle.bzip2_compress(b"", 9)[1]
    assert empty.size == 14
    one = oracle.bzip2_compress(b"\x42", 5)[1]
    text = oracle.bzip2_compress(recipes.textgen(30000, 52), 2)[1]
    for s in (empty, one, np.concatenate([text, np.frombuffer(b"garbage behind the stream", np.uint8)]),
              np.concatenate([one, np.zeros(9, np.uint8)])):
        for writes in (None, [3, 1, s.size - 4], [s.size - 1, 1]):
            rc, detail, got = same_as_one_shot(pkg, hip, oracle, s, multi, writes=writes, eager=True)
    rc, detail, got = same_as_one_shot(pkg, hip, oracle, one, multi, eager=True)
    assert rc == 0 and bytes(got) == b"\x42"


def test_80k_stream_byte_by_byte(pkg, hip, oracle):
    # 80,000 one-byte writes with a drain behind each.  Steps at every 64 KiB and at finish: an eager step per byte would be 80,000
    # GPU steps, so the eager byte-by-byte run below takes a stream of a few kB
    data = recipes.textgen(212000, 53)
    rc, stream = oracle.bzip2_compress(data, 1)
    assert rc == 0 and 70000 < stream.size < 100000
    rc, detail, got = decode(pkg, stream, 0, writes=[1] * stream.size)
    assert rc == 0 and np.array_equal(got, data)
    small = recipes.textgen(6000, 54)
    rc, stream = oracle.bzip2_compress(small, 1)
    assert rc == 0
    rc, detail, got = decode(pkg, stream, 0, writes=[1] * stream.size, eager=True)
    assert rc == 0 and np.array_equal(got, small)


def test_two_block_stream_cut_everywhere_it_matters(pkg, hip, oracle, two_blocks):
    data, stream, table = two_blocks
    b1 = table[1][0]                                  # bit where block 2 starts = first bit behind block 1
    n = stream.size
    cuts = {"in block 1's header": 4 + 9, "in block 1's data": b1 // 16, "exactly behind block 1": (b1 + 7) // 8,
            "in block 2": (b1 // 8 + n) // 2, "in the end-of-stream magic": n - 7, "in the stream crc": n - 2}
    for what, cut in cuts.items():
        piece = stream[:cut]
        for eager_cut in (None, 7, cut // 2):
            writes = None if eager_cut is None else [eager_cut, cut - eager_cut]
            rc, detail, got = same_as_one_shot(pkg, hip, oracle, piece, 0, writes=writes, eager=True)
            if what == "exactly behind block 1" and b1 % 8 == 0:
                assert rc == 0 and np.array_equal(got, data[: table[0][1]]), what
            if rc:
                assert np.array_equal(got, data[: got.size]) and got.size in (0, table[0][1], data.size), what      # whole blocks in front of the failure
    # a stream cut right behind a block succeeds, as in the reference: build one whose first block ends on a byte boundary
    for seed in range(60, 90):
        d = recipes.textgen(120000, seed)
        s = oracle.bzip2_compress(d, 1)[1]
        t = oracle.bzip2_table(s)[1]
        if len(t) == 2 and t[1][0] % 8 == 0:
            rc, detail, got = same_as_one_shot(pkg, hip, oracle, s[: t[1][0] // 8], 0, writes=[t[1][0] // 16, t[1][0] // 8 - t[1][0] // 16], eager=True)
            assert rc == 0 and np.array_equal(got, d[: t[0][1]])
            break
    else:
        raise AssertionError("no seed gives a first block that ends on a byte boundary")


# ---------------------------------------------------------------------------------------------- member boundaries
@pytest.fixture(scope="module")
def members(oracle):
    ms = [oracle.bzip2_compress(recipes.textgen(3000 + i, 54 + i), lv)[1] for i, lv in enumerate((1, 9, 3))]
    return ms, np.concatenate(ms)


@pytest.mark.parametrize("multi", [0, 1])
@pytest.mark.parametrize("tail", [b"", b"BZh9" + bytes(20)], ids=["plain", "header_and_zeros_behind"])
def test_step_boundaries_across_a_member_boundary(pkg, hip, oracle, members, multi, tail):
    ms, stream = members
    stream = np.concatenate([stream, np.frombuffer(tail, np.uint8)])
    e1 = ms[0].size
    cuts = list(range(e1 - 11, e1 + 7))               # from the first member's end-of-stream magic to behind the next header
    assert len(cuts) == 18
    rc1, detail1, want = one_shot(hip, stream, multi)
    orc, _ = oracle.bzip2_decompress(stream, multi)
    for cut in cuts:
        rc, detail, got = decode(pkg, stream, multi, writes=[cut, stream.size - cut], eager=True)
        assert (rc, detail) == (rc1, detail1) and rc == orc, (cut, rc, detail, rc1, detail1)
        if rc == 0:
            assert np.array_equal(got, want), cut


# ---------------------------------------------------------------------------------------------- damaged streams
N_DAMAGED = 140


@pytest.fixture(scope="module")
def damage_base(oracle):
    d1 = recipes.textgen(1200000, 5)
    d9 = recipes.textgen(1500000, 6)
    s1, s9 = oracle.bzip2_compress(d1, 1)[1], oracle.bzip2_compress(d9, 9)[1]
    t1 = oracle.bzip2_table(s1)[1]
    assert len(t1) >= 12
    return {"l1": (d1, s1, t1), "l9": (d9, s9, oracle.bzip2_table(s9)[1])}


def _damaged(base, i):
    """stream i of the run: (which, bytes, flipped bits, truncated?).  Every fifth is left whole; the others get 1..3 bit flips of a
    fixed seed, two thirds in the level-1 stream; every tenth is also truncated."""
    rng = np.random.default_rng(9000 + i)
    which = "l9" if i % 3 == 2 else "l1"
    s = base[which][1].copy()
    flips = []
    if i % 5:
        nf = int(rng.integers(1, 4))
        # some flips aimed at the first four bytes and the trailer, the rest anywhere
        zone = int(rng.integers(0, 12))
        for _ in range(nf):
            bit = int(rng.integers(0, 32)) if zone == 0 else int(rng.integers(s.size * 8 - 88, s.size * 8)) if zone == 1 else int(rng.integers(0, s.size * 8))
            flips.append(bit)
            s[bit >> 3] ^= 0x80 >> (bit & 7)
    trunc = i % 10 == 7
    if trunc:
        s = s[: int(rng.integers(5, s.size))]
    return which, s, sorted(flips), trunc


@pytest.mark.parametrize("group", range(10))
def test_damaged_streams(pkg, hip, oracle, damage_base, group):
    for i in range(group, N_DAMAGED, 10):
        which, s, flips, trunc = _damaged(damage_base, i)
        data, whole, table = damage_base[which]
        rc, detail, got = same_as_one_shot(pkg, hip, oracle, s, 0, chunk=65536, writes=_splits(s.size, i, 150000), read_max=200003)
        if not flips and not trunc:
            assert rc == 0
        assert np.array_equal(got, data[: got.size]), i            # always a prefix of the original
        if rc and flips and not trunc and which == "l1":
            # exactly the blocks in front of the block that holds the first flipped bit: nothing for a flip in the first four bytes,
            # every block for a flip in the trailer
            starts = [b for b, _ in table]
            k = sum(1 for b in starts if b <= flips[0]) - 1        # the block that holds it (-1: the header)
            k_end = len(starts) if flips[0] >= _eos_bit(whole) else k
            want_len = 0 if flips[0] < 32 else sum(sz for _, sz in table[: max(k_end, 0)])
            assert got.size == want_len, (i, flips, got.size, want_len)


def _eos_bit(stream):
    for b in range(stream.size * 8 - 87, stream.size * 8 - 79):
        v = 0
        for j in range(48):
            v = (v << 1) | ((int(stream[(b + j) >> 3]) >> (7 - ((b + j) & 7))) & 1)
        if v == 0x177245385090:
            return b
    raise AssertionError("no end-of-stream magic")


def test_damaged_run_is_a_real_mix(oracle, damage_base):
    codes = [oracle.bzip2_decompress(_damaged(damage_base, i)[1], 0)[0] for i in range(N_DAMAGED)]
    assert N_DAMAGED >= 120
    assert sum(1 for c in codes if c == 0) >= 25 and sum(1 for c in codes if c != 0) >= 100
    assert {0, -2, -5} <= set(codes)


# ---------------------------------------------------------------------------------------------- budgets
def _in_use():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


class _Steps:
    """counts the '[cjs dec step]' lines on stderr after every read and records the device memory in use after step 2 and last"""

    def __init__(self, capfd):
        self.capfd, self.lines, self.used = capfd, [], {}

    def __call__(self, dec):
        err = self.capfd.readouterr().err
        new = [ln for ln in err.splitlines() if ln.startswith("[cjs dec step]")]
        before = len(self.lines)
        self.lines += new
        if before < 2 <= len(self.lines):
            self.used[2] = _in_use()
        if new:
            self.used["last"] = _in_use()

    def out_bytes(self):
        return [int(ln.split(" B out")[0].split()[-1]) for ln in self.lines]


def test_output_budget_bounds_every_step(pkg, oracle, capfd):
    data = np.zeros(40000000, np.uint8)
    rc, stream = oracle.bzip2_compress(data, 1)
    assert rc == 0 and stream.size < 1000
    _in_use()
    steps = _Steps(capfd)
    rc, detail, got = decode(pkg, stream, 0, 65536, MIN_OUT, None, 8 << 20, debug=True, track=steps)
    assert rc == 0 and got.size == data.size and not got.any()
    outs = steps.out_bytes()
    print("steps %d, bytes out per step %r, in use %r" % (len(outs), outs, steps.used))
    assert len(outs) >= 4 and max(outs) <= 52 * 100000 and sum(outs) == data.size
    assert steps.used[2] == steps.used["last"]


def test_row_cap_over_2000_tiny_members(pkg, hip, oracle, capfd):
    rng = np.random.default_rng(77)
    datas = [rng.integers(97, 123, int(rng.integers(1, 301)), dtype=np.uint8) for _ in range(2000)]
    stream = np.concatenate([oracle.bzip2_compress(d, 9)[1] for d in datas])
    steps = _Steps(capfd)
    rc, detail, got = decode(pkg, stream, 1, 65536, MIN_OUT, None, 1 << 20, debug=True, track=steps)
    assert rc == 0 and np.array_equal(got, np.concatenate(datas))
    assert len(steps.lines) >= 3                       # 52 rows a step
    rc, detail, got = same_as_one_shot(pkg, hip, oracle, stream, 0)
    assert rc == 0 and np.array_equal(got, datas[0])   # only the first member; the rest is dropped


def _bz_ids():
    return [c.name for c in bz.CASES]


@pytest.mark.parametrize("name", _bz_ids())
def test_hand_built_blocks(pkg, hip, oracle, name):
    stream, want = bz.stream(oracle, bz.BY_NAME[name])
    stream = support.as_u8(stream)
    rc1, detail1, got1 = one_shot(hip, stream, 0)
    for cut in (stream.size // 3, stream.size - 9):
        cut = max(1, min(cut, stream.size - 1))
        rc, detail, got = decode(pkg, stream, 0, writes=[cut, stream.size - cut], eager=True)
        assert (rc, detail) == (rc1, detail1), (name, cut)
        if rc == 0:
            assert np.array_equal(got, got1) and bytes(got) == bytes(want), bz.first_difference(got, want)


def test_100m_golden_in_bounded_memory(pkg, capfd):
    case = support.load_golden("golden_big_bzip2_9_100m.json")["cases"][0]
    data = recipes.build(case["recipe"])
    stream = pkg.Bzip2.compressFile(data, None, 9)
    assert stream.size == case["out_len"] and support.sha256(stream) == case["out_sha256"]
    want = hashlib.sha256(data.tobytes()).hexdigest()
    del data
    _in_use()
    steps = _Steps(capfd)
    rc, detail, got = decode(pkg, stream, 0, 4 << 20, 64 << 20, [1 << 20] * (stream.size >> 20) + [stream.size & ((1 << 20) - 1)], 1 << 20,
                             debug=True, track=steps)
    print("steps %d, device bytes in use after step 2 / the last step: %r" % (len(steps.lines), steps.used))
    assert rc == 0 and got.size == case["recipe"]["n"] and hashlib.sha256(got.tobytes()).hexdigest() == want
    assert len(steps.lines) >= 5 and max(steps.out_bytes()) <= 64 << 20
    assert steps.used[2] == steps.used["last"]


@pytest.mark.slow
def test_1gib_golden_with_the_default_parameters(pkg):
    case = support.load_golden("golden_big_bzip2_9_1g.json")["cases"][0]
    data = recipes.build(case["recipe"])
    stream = pkg.Bzip2.compressFile(data, None, 9)
    want = hashlib.sha256(data.tobytes()).hexdigest()
    n = data.size
    del data
    h, n_out = hashlib.sha256(), 0
    for piece in pkg.Bzip2.decompressStream((stream[p: p + (32 << 20)] for p in range(0, stream.size, 32 << 20))):
        h.update(piece.tobytes())
        n_out += piece.size
    assert n_out == n and h.hexdigest() == want


def test_two_decoders_on_two_threads_beside_one_shot_calls(pkg, oracle):
    datas = [recipes.textgen(4000000, 31), np.concatenate([recipes.textgen(1500000, 32), np.zeros(2000000, np.uint8), recipes.textgen(700000, 33)])]
    streams = [oracle.bzip2_compress(d, lv)[1] for d, lv in zip(datas, (9, 2))]
    other = recipes.textgen(1200000, 34)
    other_stream = oracle.bzip2_compress(other, 5)[1]
    outs, errs = [None, None], []
    gate = threading.Barrier(3)

    def run(k):
        try:
            gate.wait()
            outs[k] = decode(pkg, streams[k], 0, 65536, MIN_OUT, _splits(streams[k].size, 40 + k, 200000), 50000)
        except BaseException as e:      # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    gate.wait()
    mids = [(pkg.Bzip2.decompressFile(other_stream), pkg.Bzip2.compressFile(other, None, 5)) for _ in range(2)]
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        assert outs[k][0] == 0 and np.array_equal(outs[k][2], datas[k]), k
    for back, again in mids:
        assert np.array_equal(back, other) and np.array_equal(again, other_stream)


def test_python_generator(pkg, oracle):
    data = recipes.textgen(1800000, 41)
    rc, stream = oracle.bzip2_compress(data, 3)
    assert rc == 0
    cuts = [0, 1, 3, 3, 70000, 300000, 300001, stream.size]
    chunks = [bytes(stream[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pieces = list(pkg.Bzip2.decompressStream(iter(chunks), False, 65536, MIN_OUT))
    assert len(pieces) > 1
    assert np.array_equal(np.concatenate(pieces), data)
    bad = stream.copy()
    bad[stream.size // 2] ^= 4
    got = []
    with pytest.raises(pkg.CjsError) as e:
        for p in pkg.Bzip2.decompressStream([bad[:100000], bad[100000:]], False, 65536, MIN_OUT):
            got.append(p)
    with pytest.raises(pkg.CjsError) as e1:
        pkg.Bzip2.decompressFile(bad)
    assert str(e.value) == str(e1.value)
    got = np.concatenate(got) if got else np.empty(0, np.uint8)
    assert 0 < got.size < data.size and np.array_equal(got, data[: got.size])


# ---------------------------------------------------------------------------------------------- JS fronts
NODE = shutil.which("node")


def _sample5():
    g = support.load_golden("golden_small.json")
    case = [c for c in g["cases"] if c["algo"] == "Bzip2" and c["name"] == "sample5" and c["level"] == 9][0]
    ref = os.path.join(recipes.DATA, "sample5.ref")
    return case, ref


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_front_streams_in_and_out(pkg, oracle):
    case, ref = _sample5()
    data = np.fromfile(ref, dtype=np.uint8)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    assert support.sha256(stream) == case["out_sha256"]
    bad = stream.copy()
    bad[stream.size * 2 // 3] ^= 0x10
    rc, table = oracle.bzip2_table(stream)
    assert rc == 0 and len(table) > 2
    starts = [b for b, _ in table]
    k = sum(1 for b in starts if b <= (stream.size * 2 // 3) * 8 + 3) - 1
    in_front = sum(sz for _, sz in table[:k])
    tmp = tempfile.mkdtemp()
    good_path, bad_path = os.path.join(tmp, "good.bz2"), os.path.join(tmp, "bad.bz2")
    stream.tofile(good_path)
    bad.tofile(bad_path)
    script = r"""
      const fs = require('fs'), crypto = require('crypto');
      const m = require(process.argv[1]);
      const data = fs.readFileSync(process.argv[2]), bad = fs.readFileSync(process.argv[3]);
      const sha = (b) => crypto.createHash('sha256').update(Buffer.from(b)).digest('hex');
      const r = {};
      let pos = 0;
      const inS = { readByte: function () { return pos < data.length ? data[pos++] : -1; } };
      const a = m.Bzip2.decompressFile(inS);
      r.readbyte = sha(a); r.readbyte_len = a.length;
      let p2 = 0;
      const inR = { readByte: function () { return p2 < data.length ? data[p2++] : -1; },
                    read: function (buf, off, len) { const n = Math.min(len, data.length - p2, 300001); data.copy(Buffer.from(buf.buffer, buf.byteOffset + off, n), 0, p2, p2 + n); p2 += n; return n; } };
      r.read_api = sha(m.Bzip2.decompressFile(inR));
      const chunks = [];
      const outS = { writeByte: function (b) { chunks.push(b); } };
      r.returned = m.Bzip2.decompressFile(data, outS) === outS;
      r.sink = sha(Uint8Array.from(chunks)); r.sink_len = chunks.length;
      r.buffer = sha(m.Bzip2.decompressFile(data));
      const got = [];
      try { m.Bzip2.decompressFile(bad, { writeByte: function (b) { got.push(b); } }); r.threw = null; }
      catch (e) { r.threw = e.message; r.type = e.constructor.name; r.code = e.errorCode; }
      r.bad_sink = sha(Uint8Array.from(got)); r.bad_sink_len = got.length;
      try { m.Bzip2.decompressFile(bad); r.one_shot = null; } catch (e) { r.one_shot = e.message; }
      console.log(JSON.stringify(r));
    """
    env = dict(os.environ, CJS_DEC_CHUNK_BYTES="65536")
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "compressjs-flattened_amd", "js", "index.js"), good_path, bad_path],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    want = support.sha256(data)
    assert r["readbyte_len"] == data.size and r["readbyte"] == want and r["read_api"] == want and r["buffer"] == want
    assert r["returned"] is True and r["sink_len"] == data.size and r["sink"] == want
    # the reference's message, and the sink holds exactly the blocks in front of the failure
    assert r["threw"] is not None and r["threw"] == r["one_shot"] and r["type"] == "TypeError" and r["code"] == -5
    assert r["threw"].startswith("Data error: Bad block CRC")
    assert r["bad_sink_len"] == in_front and r["bad_sink"] == support.sha256(data[:in_front])


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_cli_streams_file_and_pipe(pkg):
    case, ref = _sample5()
    data = np.fromfile(ref, dtype=np.uint8)
    cli = os.path.join(ROOT, "compressjs-flattened_amd", "js", "cli.js")
    tmp = tempfile.mkdtemp()
    src, dst = os.path.join(tmp, "in.bz2"), os.path.join(tmp, "out")
    np.array(pkg.Bzip2.compressFile(data, None, 9)).tofile(src)
    env = dict(os.environ, CJS_DEBUG="1", CJS_DEC_CHUNK_BYTES="65536")
    o = subprocess.run([NODE, cli, "-d", "-t", "bzip2", src, dst], capture_output=True, timeout=600, env=env)
    assert o.returncode == 0, o.stderr[-2000:]
    got = np.fromfile(dst, dtype=np.uint8)
    assert got.size == data.size and np.array_equal(got, data)
    steps = [ln for ln in o.stderr.decode().splitlines() if ln.startswith("[cjs dec step]")]
    assert len(steps) > 1, o.stderr[-2000:]                   # one line per step; the stream is larger than the chunk
    with open(src, "rb") as f:
        p = subprocess.run("cat | %s %s -d -t bzip2" % (NODE, cli), shell=True, stdin=f, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    b = np.frombuffer(p.stdout, dtype=np.uint8)
    assert b.size == data.size and np.array_equal(b, data)
