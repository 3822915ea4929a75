"""The line keys on the GPU (cjs_bzip2_line_keys[_device], Bzip2Index.line_keys / diff_stream, LineDiff.normal_text): every record of
every line against the key restated with Python's big integers over the decoded text (linekeys_cases.text_keys) -- across 16-byte
vectors, 1 KiB rows, 16 KiB tiles and blocks, blocks of a few bytes, runs of newlines, a line over several tiles and over several
whole blocks, windows, caps, passes, batches, a damaged block, a foreign and a wrong table -- and the diff of two streams end to
end.  Every case runs the host form and the device form (linekeys_cases.both_forms)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import linekeys_cases as lk
import lines_cases as lc
import range_cases as rg

pytestmark = pytest.mark.gpu

NAMES = ("F1", "LN2", "LN3", "CR1", "CR2", "CR3")
SEEDS = (0, 0xFEEDFACE12345678)
SEAMS = (16, 1024, 16384)


@pytest.fixture(scope="module")
def L():
    return lk.bind()


def _members(oracle, pieces):
    """the pieces as the members of one multistream file, levels cycling 1..9"""
    parts = []
    for k, p in enumerate(pieces):
        rc, s = oracle.bzip2_compress(np.frombuffer(p, dtype=np.uint8), 1 + k % 9)
        assert rc == 0
        parts.append(np.asarray(s, dtype=np.uint8))
    return np.concatenate(parts), np.frombuffer(b"".join(pieces), dtype=np.uint8), 1


def crafted(name, oracle):
    if name == "CR1":      # members of 1..8 bytes without a newline (one line over eight whole blocks), a member without a block, a line over three whole blocks
        return _members(oracle, [b"abcdefgh"[:k] for k in range(1, 9)] + [b"x\n", b"", b"q", b"rs", b"tuv", b"\nend of it\n\n", b"tail"])
    if name == "CR2":      # only newlines: a few, one, more than a tile of them
        return _members(oracle, [b"\n" * 5, b"\n", b"\n" * 17000])
    return _members(oracle, [b""])      # CR3: a stream without a block


def _fixture(L, name, oracle):
    if name == "F1":
        stream, plain, multi, _ = rg.f1()
    elif name == "LN2":
        stream, plain, multi = lc.ln2(oracle)
    elif name == "LN3":
        stream, plain, multi = lc.ln3(oracle)[:2] + (0,)
    else:
        stream, plain, multi = crafted(name, oracle)
    rc, h = rg.build(L, stream, multi)
    assert rc == 0, (name, rc, rg.detail(L))
    e = rg.entries(L, h)
    bounds = np.concatenate([[0], np.cumsum([x[2] for x in e])]).astype(np.int64)
    f = dict(name=name, stream=stream, plain=plain, h=h, entries=e, bounds=bounds, nl=lc.newlines(plain), total=int(plain.size), multi=multi)
    f["dev"] = lc.on_device(stream)
    return f


@pytest.fixture(scope="module")
def fx(L, oracle):
    out = {name: _fixture(L, name, oracle) for name in NAMES}
    for f in out.values():
        f["t"] = lc.build_both(L, f["stream"], f["h"], f["dev"])
        f["want"] = {seed: lk.text_keys(f["plain"].tobytes(), seed) for seed in SEEDS}      # computed once, shared, never changed
        assert len(f["want"][0]) == f["nl"].size + 1
    return out


def seam_lines(f):
    """{seam: the lines whose bytes cross it}: for 16, 1024 and 16384 a line with bytes on both sides of a multiple of that, counted
    from its block's first byte; for "block" a line with bytes in two blocks.  From the fixture's own bounds."""
    nl, total, b = f["nl"], f["total"], f["bounds"]
    out = {s: [] for s in SEAMS + ("block",)}
    starts = np.concatenate([[0], nl + 1]).astype(np.int64)          # start(k), k = 0 .. N
    ends = np.concatenate([nl + 1, [total]]).astype(np.int64)         # start(k + 1)
    for B0, B1 in zip(b[:-1], b[1:]):
        if B1 == B0:
            continue
        if 0 < B0 < total:
            k = int(np.searchsorted(starts, B0, "right")) - 1       # the line that holds byte B0
            if starts[k] < B0 < ends[k]:
                out["block"].append(k)
        for s in SEAMS:
            for at in range(int(B0) + s, int(B1), s):
                k = int(np.searchsorted(starts, at, "right")) - 1
                if starts[k] < at < ends[k] and starts[k] >= B0:
                    out[s].append(k)
    return {s: sorted(set(v)) for s, v in out.items()}


def test_the_fixtures_hold_what_the_kernels_can_get_wrong(fx):
    for name, kinds in (("F1", SEAMS + ("block",)), ("LN3", SEAMS), ("LN2", ("block",)), ("CR1", ("block",))):
        s = seam_lines(fx[name])
        assert all(len(s[k]) >= 1 for k in kinds), (name, {k: len(v) for k, v in s.items()})
    f = fx["LN3"]
    long_line = lc.number(f["nl"], f["total"], lc.LN3_QUIET[0])
    assert lc.start(f["nl"], f["total"], long_line + 1) - lc.start(f["nl"], f["total"], long_line) > 2 * 16384      # a line over several tiles
    for name, least in (("LN2", 4), ("CR1", 8)):      # a line over whole blocks
        f = fx[name]
        assert max(lc.blocks_of_line(f["nl"], f["total"], f["bounds"], k) for k in range(f["nl"].size + 1)) >= least
    assert fx["CR2"]["nl"].size == fx["CR2"]["total"] == 17006 and fx["CR3"]["total"] == 0 and len(fx["CR3"]["entries"]) == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_every_line(L, fx, name, seed):
    f = fx[name]
    got, info, d = lk.both_forms(L, f["stream"], f["h"], f["t"], f["dev"], seed=seed)
    want = f["want"][seed]
    assert len(got) == len(want) and info == (len(want), 0, lk.M64, sum(1 for e in f["entries"] if e[2])) and d == ""
    assert got == want, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def windows(f):
    N = int(f["nl"].size)
    w = [(0, 0), (0, 1), (N, 1), (N, 5), (N + 1, 3), (N + 7, lk.M64), (0, lk.M64), (1, lk.M64), (3, lk.M64 - 1), (lk.M64, lk.M64), (0, N), (0, N + 1)]
    for kind, ks in seam_lines(f).items():
        for k in ks[:2] + ks[-1:]:
            w += [(k, 1), (k, 3), (max(k - 2, 0), min(k, 2) + 1), (k + 1, 2), (max(k - 1, 0), 1)]      # the seam line first, last, alone, just outside
    return w


@pytest.mark.parametrize("name", NAMES)
def test_windows(L, fx, name):
    f = fx[name]
    want_all = f["want"][SEEDS[1]]
    n_all = len(want_all)
    for first, count in windows(f):
        want = want_all[first:min(first + count, n_all)] if first < n_all else []
        got, info, d = lk.both_forms(L, f["stream"], f["h"], f["t"], f["dev"], first=first, count=count, seed=SEEDS[1])
        assert info[0] == len(want) and got == want and info[1] == 0, (first, count)


@pytest.mark.parametrize("name", ("F1", "LN2", "CR1"))
def test_caps(L, fx, name):
    f = fx[name]
    want = f["want"][0]
    for first, count, cap in ((0, lk.M64, 1), (0, lk.M64, len(want) - 1), (2, 7, 3), (2, 7, 7), (2, 7, 20), (len(want) - 1, 9, 1), (5, 0, 4)):
        in_window = want[first:first + count]
        got, info, d = lk.both_forms(L, f["stream"], f["h"], f["t"], f["dev"], first=first, count=count, cap=cap)      # (nothing past min(cap, n) is written: _unguard)
        assert info[0] == len(in_window) and got == in_window[:cap], (first, count, cap)
    # the count query: the table alone, no block touched
    rc, keys, info = lk._keys_call(L.cjs_bzip2_line_keys, f["stream"].ctypes.data_as(rg.u8p), f["stream"].size, f["h"], f["t"], 0, lk.M64, 0, 0)
    assert rc == 0 and info.n_lines == len(want) and info.blocks_decoded == 0


def digest(got, info, d):
    return [hashlib.sha256(lk.key_array(got).tobytes()).hexdigest(), list(info), d]


def child(names, env):
    """(the child of the two tests below) the fixtures `names` under the environment `env`: {name/setting: digest of all keys and
    of one window}; the [cjs linekeys] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    for k, v in env.items():
        if k != "CJS_RANGE_PASS_BLOCKS":
            os.environ[k] = v
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = lk.bind(), support.Oracle(), {}
    for name in names:
        f = _fixture(L, name, oracle)
        os.environ["CJS_RANGE_PASS_BLOCKS"] = "0"
        t = lc.build_both(L, f["stream"], f["h"], f["dev"])
        for cap in env.get("CJS_RANGE_PASS_BLOCKS", "0").split(","):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            out[name + "/" + cap] = _digests(L, f, t)
    print(json.dumps(out))


def _digests(L, f, t):
    N = int(f["nl"].size)
    return [digest(*lk.both_forms(L, f["stream"], f["h"], t, f["dev"], seed=SEEDS[1])),
            digest(*lk.both_forms(L, f["stream"], f["h"], t, f["dev"], first=N // 3, count=N // 2, seed=5))]


LINE = r"\[cjs linekeys\] (host|device): lines \[(\d+), (\d+)\), (\d+) of \d+ blocks touched, (\d+) bad, (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\)"


def _run_child(names, env):
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_linekeys as t; t.child(%r, %r)" % (names, env)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=penv,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [(form, int(a), int(b), int(t), int(bad), int(p), int(bt)) for form, a, b, t, bad, p, bt in re.findall(LINE, run.stderr)]
    return json.loads(run.stdout.strip().splitlines()[-1]), lines


def test_several_passes_give_the_one_pass_records(L, fx):
    got, lines = _run_child(["F1", "LN2"], {"CJS_RANGE_PASS_BLOCKS": "1,2,3"})
    for name in ("F1", "LN2"):
        here = _digests(L, fx[name], fx[name]["t"])
        assert here[0][0] == hashlib.sha256(lk.key_array(fx[name]["want"][SEEDS[1]]).tobytes()).hexdigest()
        for cap in ("1", "2", "3"):
            assert got[name + "/" + cap] == here, (name, cap)
    # not vacuous: a pass held at most `cap` of the touched blocks; per fixture and cap two calls with keys in either form (the
    # count queries print nothing: they return before the window is looked at)
    assert len(lines) == 24, lines
    for i, (form, a, b, t, bad, p, bt) in enumerate(lines):
        cap = (1, 2, 3)[(i // 4) % 3]
        assert form == ("host", "device")[i % 2] and t >= 4 and bad == 0 and p == (t + cap - 1) // cap, (i, lines[i])


def test_several_batches_in_a_pass_give_the_same(L, fx):
    """F1 with at most 250,000 BWT bytes to an inverse-BWT batch (two blocks): lines that span batches are joined on the host"""
    got, lines = _run_child(["F1"], {"CJS_DEC_BATCH_ELEMS": "250000"})
    assert got["F1/0"] == _digests(L, fx["F1"], fx["F1"]["t"])
    assert len(lines) == 4 and all(p == 1 and bt >= 3 for form, a, b, t, bad, p, bt in lines), lines
    assert lines[0][3] == 10


def test_damage(L, fx):
    """LN2 with one bit flipped in one block (the lowest bit of its BWT start): the lines the table gives that block, and the one
    that goes on behind it, are all-ones; every other record is unchanged; info and the detail name the block"""
    f = fx["LN2"]
    e, b, nl, total, plain = f["entries"], f["bounds"], f["nl"], f["total"], f["plain"]
    want = f["want"][0]
    counts = lc.block_counts(plain, b)
    cum = np.concatenate([[0], np.cumsum(counts)])
    text = lambda k: plain[b[k]:b[k + 1]].tobytes()
    turned = lambda k: any(text(k)[r:] + text(k)[:r] == text(k) for r in range(1, len(text(k))))      # (a rotation of itself: another BWT start decodes to the same bytes)
    inner = [k for k in range(3, len(e) - 3) if e[k][2] >= 3 and counts[k] >= 1 and not turned(k)]
    open_end = next(k for k in inner if plain[b[k + 1] - 1] != 10)          # its last line goes on in the next block
    shut_end = next(k for k in inner if plain[b[k + 1] - 1] == 10)          # its last byte is a newline
    for blk in (open_end, shut_end):
        damaged = f["stream"].copy()
        bit = e[blk][0] + 48 + 32 + 1 + 23
        damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
        dev = lc.on_device(damaged)
        got, info, d = lk.both_forms(L, damaged, f["h"], f["t"], dev)
        touched = [lc.number(nl, total, int(b[blk])), lc.number(nl, total, int(b[blk + 1]) - 1)]      # the lines of its first and last byte
        bad = set(range(int(cum[blk]), int(cum[blk + 1]) + 1))
        if blk == open_end:
            assert bad == set(range(touched[0], touched[1] + 1)), "exactly the lines with a byte in the block"
        else:                                               # the table cannot say that the block ends in a newline: one line more
            assert bad == set(range(touched[0], touched[1] + 2))
        assert [k for k, g in enumerate(got) if g == lk.ONES] == sorted(bad)
        assert all(g == w for k, (g, w) in enumerate(zip(got, want)) if k not in bad) and len(got) == len(want)
        assert info == (len(want), 1, blk, sum(1 for x in e if x[2]))
        assert re.fullmatch(r"Bad block CRC \(got [0-9a-f]+ expected %x\)" % e[blk][3], d) or d == "index does not match the stream at block %d" % blk, d
        # a window that ends in front of the block does not touch it
        got, info, d = lk.both_forms(L, damaged, f["h"], f["t"], dev, first=0, count=int(cum[blk - 1]))
        assert got == want[:int(cum[blk - 1])] and info[1] == 0 and d == ""


def test_tables_that_are_not_the_streams(L, fx):
    f, other = fx["F1"], fx["LN2"]
    for fn, src in ((L.cjs_bzip2_line_keys, f["stream"].ctypes.data_as(rg.u8p)), (L.cjs_bzip2_line_keys_device, f["dev"][1])):
        rc, keys, info = lk._keys_call(fn, src, f["stream"].size, f["h"], other["t"], 0, lk.M64, 0, 4)
        assert rc == rg.E_INVALID and rg.detail(L) == lc.FOREIGN
    # one count moved between neighbouring blocks: the totals still agree with the index, the stream does not
    wrong = lc.block_counts(f["plain"], f["bounds"])
    wrong[2] += 1; wrong[3] -= 1
    rc, t = lc.create(L, f["h"], wrong)
    assert rc == 0
    for call in (lambda **kw: lk.keys_host(L, f["stream"], f["h"], t, **kw), lambda **kw: lk.keys_device(L, f["dev"][1], f["stream"].size, f["h"], t, **kw)):
        rc, keys, info, d = call()
        assert rc == rg.E_DATA and d == lk.MISMATCH % 2 and keys.size == 0
        rc, keys, info, d = call(first=0, count=int(sum(wrong[:2])) - 5)      # a window in front of block 2 is served
        assert rc == 0 and lk.as_tuples(keys) == f["want"][0][:int(sum(wrong[:2])) - 5]
    L.cjs_bzip2_lines_destroy(t)


def test_argument_errors(L, fx):
    f = fx["LN2"]
    src, n = f["stream"].ctypes.data_as(rg.u8p), f["stream"].size
    k = np.zeros(4, dtype=lk.KEY)
    info = lk.KeysInfo()
    ok = (src, n, f["h"], f["t"], 0, 4, 0, k.ctypes.data, 4, info, None)
    for at, value in ((0, None), (1, n - 1), (2, None), (3, None), (7, None), (9, None)):
        a = list(ok)
        a[at] = value
        a[9] = ctypes_ref(a[9])
        assert L.cjs_bzip2_line_keys(*a) == rg.E_INVALID, at
    a = list(ok)
    a[9] = ctypes_ref(info)
    assert L.cjs_bzip2_line_keys(*a) == 0 and info.n_lines == 4


def ctypes_ref(x):
    import ctypes
    return ctypes.byref(x) if x is not None else None


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("compressjs-flattened_amd")


def _edited(lines, at, rng):
    """`lines` with, around every line number in `at`, one line changed, one deleted or one inserted"""
    out, at = [], sorted(set(at))
    for k, ln in enumerate(lines):
        kind = at.index(k) % 3 if k in at else -1
        if kind == 0:
            out.append(b"changed %d\n" % k)
        elif kind == 2:
            out += [b"inserted %d\n" % k, ln]
        elif kind == -1:
            out.append(ln)
    return out


def _apply_normal(text, a_lines):
    """what `patch` does with a normal-format diff: -> the new lines (a last line without a newline as the marker says)"""
    out, at = [], 0
    rows = text.split(b"\n")[:-1]
    i = 0
    while i < len(rows):
        m = re.fullmatch(rb"(\d+)(?:,(\d+))?([acd])(\d+)(?:,(\d+))?", rows[i])
        assert m, rows[i]
        a0, a1, cmd, b0, b1 = int(m.group(1)), int(m.group(2) or m.group(1)), m.group(3), int(m.group(4)), int(m.group(5) or m.group(4))
        i += 1
        take = a0 if cmd == b"a" else a0 - 1
        out += a_lines[at:take]
        at = take if cmd == b"a" else a1
        if cmd != b"a":
            for k in range(a0 - 1, a1):
                assert rows[i] == b"< " + a_lines[k].rstrip(b"\n"), (rows[i], a_lines[k])
                i += 1
                if i < len(rows) and rows[i].startswith(b"\\"):
                    assert not a_lines[k].endswith(b"\n")
                    i += 1
        if cmd == b"c":
            assert rows[i] == b"---"
            i += 1
        if cmd != b"d":
            for k in range(b0, b1 + 1):
                assert rows[i].startswith(b"> ")
                out.append(rows[i][2:] + b"\n")
                i += 1
                if i < len(rows) and rows[i].startswith(b"\\"):
                    out[-1] = out[-1][:-1]
                    i += 1
    return out + a_lines[at:]


def _stream_of(oracle, pkg, text, level):
    rc, s = oracle.bzip2_compress(np.frombuffer(text, dtype=np.uint8), level)
    assert rc == 0
    s = np.asarray(s, dtype=np.uint8)
    ix = pkg.Bzip2Index.build(s)
    return s, ix, pkg.Bzip2Lines.build(s, ix)


def _real_lines(text):
    return [x for x in lk.split_lines(text) if x]          # (the empty final line is no line of `diff`'s)


@pytest.mark.parametrize("variant", ("whole", "short", "no final newline"))
def test_diff_stream(L, fx, pkg, oracle, variant):
    f = fx["F1"]
    a_lines = _real_lines(f["plain"].tobytes())
    seams = seam_lines(f)
    at = [k for kind in seams.values() for k in kind[:3] + kind[-2:]] + [0, 1, len(a_lines) - 1]
    rng = np.random.RandomState(3)
    if variant == "whole":                                  # A is F1 as it is (level 1); B at level 9: its blocks fall elsewhere
        a_stream, b_level = f["stream"], 9
    else:                                                   # at most 400 lines, so that the DP can say what the minimum is
        a_lines = a_lines[:400]
        at = [0, 1, 7, 8, 9, 150, 151, 399] + rng.randint(10, 390, 12).tolist()
        if variant == "no final newline":
            a_lines[-1] = a_lines[-1][:-1]
        rc, s = oracle.bzip2_compress(np.frombuffer(b"".join(a_lines), dtype=np.uint8), 3)
        assert rc == 0
        a_stream, b_level = np.asarray(s, dtype=np.uint8), 7
    b_lines = _edited(a_lines, [k for k in at if k < len(a_lines)], rng)
    if variant == "no final newline":
        b_lines[-1] = b_lines[-1] if b_lines[-1].endswith(b"\n") else b_lines[-1] + b"\n"      # B's last line has its newline, A's has not
    ia = pkg.Bzip2Index.build(a_stream)
    la = pkg.Bzip2Lines.build(a_stream, ia)
    b_stream, ib, lb = _stream_of(oracle, pkg, b"".join(b_lines), b_level)
    if variant == "whole":
        assert ib.blocks != ia.blocks
    res = ia.diff_stream(a_stream, la, b_stream, ib, lb, seed=11)
    assert res.minimal and not res.equal and res.hunks
    assert lk.apply_hunks(a_lines, b_lines, res.hunks) == b_lines
    assert res.edits == sum(h[1] + h[3] for h in res.hunks) and res.common == (len(a_lines) + len(b_lines) - res.edits) // 2
    if variant != "whole":
        assert res.edits == lk.edit_distance(a_lines, b_lines)
    text = res.normal_text(ia, a_stream, la, ib, b_stream, lb)
    assert _apply_normal(text, a_lines) == b_lines
    if variant == "no final newline":
        assert text.count(b"\\ No newline at end of file\n") == 1 and text.endswith(b"\n")
    # the same stream against itself; the key arrays through diff_keys and the device form
    same = ia.diff_stream(a_stream, la, a_stream, ia, la)
    assert same.equal and same.hunks == [] and same.edits == 0 and same.common == len(a_lines) and same.normal_text(ia, a_stream, la, ia, a_stream, la) == b""
    keep, ptr = lc.on_device(b_stream)
    kb, info = pkg.line_keys_device(ptr, b_stream.size, ib, lb, seed=11)
    ka, _ = ia.line_keys(a_stream, la, seed=11)
    assert info.n_lines == kb.size and info.bad_blocks == 0
    if variant != "whole":
        assert lk.as_tuples(kb) == lk.text_keys(b"".join(b_lines), 11)
    drop = lambda k: k[:-1] if k[-1].tolist() == (0, 0, 0) else k
    assert pkg.diff_keys(drop(ka), drop(kb)).hunks == res.hunks


def test_diff_stream_on_damage(fx, pkg):
    f = fx["F1"]
    ix = pkg.Bzip2Index.build(f["stream"])
    ln = pkg.Bzip2Lines.build(f["stream"], ix)
    damaged = f["stream"].copy()
    rg.set_bits(damaged, f["entries"][7][0], 48, 0x314159265358)
    for a, b in ((damaged, f["stream"]), (f["stream"], damaged)):
        with pytest.raises(pkg.CjsError) as e:
            ix.diff_stream(a, ln, b, ix, ln)
        assert e.value.errorCode == rg.E_DATA and "block 7" in str(e.value)
    keys, info = ix.line_keys(damaged, ln)
    assert info.bad_blocks == 1 and info.first_bad_block == 7 and "block 7" in info.detail
    bad = [k for k, g in enumerate(lk.as_tuples(keys)) if g == lk.ONES]
    counts = ln.counts()
    cum = np.concatenate([[0], np.cumsum(counts)])
    assert bad == list(range(int(cum[7]), int(cum[8]) + 1))
