"""The line table on the GPU (cjs_bzip2_lines_*, Bzip2Lines, Bzip2Index.line_starts / line_numbers / read_lines / grep_lines): every
count, start(k) and number(o) against numpy on the decoded text -- across block seams, blocks of a few bytes, tile and row seams,
long lines, runs of newlines, the bytes a SWAR test may take for a newline, passes, batches and damaged blocks.  Every case runs
the host form and the device form (lines_cases.both_forms)."""
import bisect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lines_cases as lc
import range_cases as rg
import search_cases as sc

pytestmark = pytest.mark.gpu

NAMES = ("F1", "LN2", "LN3")


@pytest.fixture(scope="module")
def L():
    return lc.bind()


def _fixture(L, name, oracle):
    extra = {}
    if name == "F1":
        stream, plain, multi, _ = rg.f1()
    elif name == "LN2":
        stream, plain, multi = lc.ln2(oracle)
    else:
        stream, plain, want_bounds, pairs, highs = lc.ln3(oracle)
        multi, extra = 0, dict(pairs=pairs, highs=highs, want_bounds=want_bounds)
    rc, h = rg.build(L, stream, multi)
    assert rc == 0, (name, rc, rg.detail(L))
    e = rg.entries(L, h)
    bounds = np.concatenate([[0], np.cumsum([x[2] for x in e])]).astype(np.int64)
    if "want_bounds" in extra:
        assert bounds.tolist() == extra["want_bounds"].tolist()
    f = dict(name=name, stream=stream, plain=plain, h=h, entries=e, bounds=bounds, nl=lc.newlines(plain), total=int(plain.size), multi=multi, **extra)
    f["dev"] = lc.on_device(stream)
    return f


@pytest.fixture(scope="module")
def fx(L, oracle):
    out = {name: _fixture(L, name, oracle) for name in NAMES}
    for f in out.values():
        f["t"] = lc.build_both(L, f["stream"], f["h"], f["dev"])
    return out


def _seams(f):
    """decoded offsets where a block, a 16 KiB tile of a block or (LN3) a 1 KiB row starts"""
    b = f["bounds"]
    at = set(int(x) for x in b)
    for lo, hi in zip(b[:-1], b[1:]):
        at |= set(range(int(lo), int(hi), lc.TILE))
        if f["name"] == "LN3":
            at |= set(range(int(lo), int(hi), lc.ROW))
    if f["name"] == "LN3":
        at |= set(range(0, f["total"], lc.ROW))
    return sorted(at)


def locate_questions(f):
    nl, total, N = f["nl"], f["total"], int(f["nl"].size)
    ks = [0, 1, 2, N - 1, N, N + 1, lc.TOP]
    for T in _seams(f):                                     # the lines whose newline is the last byte in front of a seam or the first behind it
        i = int(np.searchsorted(nl, T - 1, "left"))
        ks += [i, i + 1, i + 2]
    if f["name"] == "LN3":
        w0, w1 = lc.LN3_WHITE
        first = int(np.searchsorted(nl, w0, "left")) + 1
        ks += list(range(first - 1, first + (w1 - w0) + 1))  # every line of the newline stretch
        q0, q1 = lc.LN3_QUIET
        ks += [int(np.searchsorted(nl, q0 - 1, "left")) + 1, int(np.searchsorted(nl, q1, "left")) + 1]      # the long line, the line after it
    rng = np.random.RandomState(11)
    r = rng.randint(0, N + 2, 2000).tolist()
    ks += sorted(r, reverse=True) + rng.permutation(r).tolist()
    return [min(max(int(k), 0), lc.TOP) for k in ks]


def number_questions(f):
    total = f["total"]
    os_ = [0, total - 1, total, total + 7, lc.TOP]
    for T in _seams(f):
        os_ += [T - 1, T, T + 1]
    for p in f.get("pairs", []) + f.get("highs", []):
        os_ += [p, p + 1, p + 2]
    os_ += np.random.RandomState(12).randint(0, total + 2, 2000).tolist()
    return [int(o) for o in os_ if o >= 0]


def _starts(f, ks):
    return [lc.start(f["nl"], f["total"], k) for k in ks]


def _numbers(f, os_):
    return [lc.number(f["nl"], f["total"], o) for o in os_]


@pytest.mark.parametrize("name", NAMES)
def test_build(L, fx, name):
    f = fx[name]
    want = lc.block_counts(f["plain"], f["bounds"])
    assert lc.counts(L, f["t"]) == want and lc.info(L, f["t"]) == (len(want), int(f["nl"].size), f["total"])
    raw = lc.save(L, f["t"])
    assert raw == lc.image(want, f["total"], lc.crc_fold(f["entries"]))
    rc, t2 = lc.load(L, raw, f["h"])
    assert rc == 0 and lc.counts(L, t2) == want and lc.info(L, t2) == lc.info(L, f["t"]) and lc.save(L, t2) == raw
    L.cjs_bzip2_lines_destroy(t2)
    if name == "F1":
        assert f["total"] == 938848 and f["nl"].size == 99171 and len(want) == 10 and f["plain"][-1] == 10 and int(np.diff(f["nl"]).max()) <= 24


@pytest.mark.parametrize("name", NAMES)
def test_locate(L, fx, name):
    f = fx[name]
    ks = locate_questions(f)
    got, st, d = lc.both_forms(L, "locate", f["stream"], f["h"], f["t"], ks, f["dev"])
    assert not any(st) and d == ""
    want = _starts(f, ks)
    assert got == want, [(k, g, w) for k, g, w in zip(ks, got, want) if g != w][:10]
    at = set(f["nl"].tolist())                              # not vacuous: a newline stands on both sides of an inner block seam
    if name != "F1":
        assert any(int(B) - 1 in at and int(B) in at for B in f["bounds"][1:-1])


@pytest.mark.parametrize("name", NAMES)
def test_number(L, fx, name):
    f = fx[name]
    os_ = number_questions(f)
    got, st, d = lc.both_forms(L, "number", f["stream"], f["h"], f["t"], os_, f["dev"])
    assert not any(st) and d == ""
    want = _numbers(f, os_)
    assert got == want, [(o, g, w) for o, g, w in zip(os_, got, want) if g != w][:10]


def table_questions(f):
    """questions the table alone answers"""
    N = int(f["nl"].size)
    starts = sorted(set(int(b) for b, e in zip(f["bounds"][:-1], f["bounds"][1:]) if e > b))
    return [0, N + 1, N + 9, lc.TOP], starts + [f["total"], f["total"] + 7, lc.TOP]


def child(names, env):
    """(the child of the two tests below) the fixtures `names` under the environment `env`: {name/setting: [counts, starts,
    numbers]}, then one call of each kind that the table alone answers; the [cjs lines] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    for k, v in env.items():
        if k != "CJS_RANGE_PASS_BLOCKS":
            os.environ[k] = v
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = lc.bind(), support.Oracle(), {}
    for name in names:
        f = _fixture(L, name, oracle)
        for cap in env.get("CJS_RANGE_PASS_BLOCKS", "0").split(","):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            t = lc.build_both(L, f["stream"], f["h"], f["dev"])
            starts = lc.both_forms(L, "locate", f["stream"], f["h"], t, locate_questions(f), f["dev"])
            numbers = lc.both_forms(L, "number", f["stream"], f["h"], t, number_questions(f), f["dev"])
            out[name + "/" + cap] = [lc.counts(L, t), list(starts), list(numbers)]
    sys.stderr.write("table only\n")
    ks, os_ = table_questions(f)
    out["table"] = [list(lc.both_forms(L, "locate", f["stream"], f["h"], t, ks, f["dev"])), list(lc.both_forms(L, "number", f["stream"], f["h"], t, os_, f["dev"]))]
    print(json.dumps(out))


LINE = r"\[cjs lines\] (host|device): (build|locate|number), (\d+) queries, (\d+) of \d+ blocks touched, (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\)"


def _run_child(names, env):
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_lines as t; t.child(%r, %r)" % (names, env)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=penv,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    work, table = run.stderr.split("table only\n")
    parse = lambda text: [(form, kind, int(q), int(t), int(p), int(b)) for form, kind, q, t, p, b in re.findall(LINE, text)]
    return json.loads(run.stdout.strip().splitlines()[-1]), parse(work), parse(table)


def _here(L, f):
    ks, os_ = locate_questions(f), number_questions(f)
    starts = lc.both_forms(L, "locate", f["stream"], f["h"], f["t"], ks, f["dev"])
    numbers = lc.both_forms(L, "number", f["stream"], f["h"], f["t"], os_, f["dev"])
    assert starts[0] == _starts(f, ks) and numbers[0] == _numbers(f, os_)
    return [lc.counts(L, f["t"]), list(starts), list(numbers)]


def test_several_passes_give_the_one_pass_answers(L, fx):
    got, lines, table = _run_child(["F1", "LN2"], {"CJS_RANGE_PASS_BLOCKS": "1,3"})
    for name in ("F1", "LN2"):
        here = _here(L, fx[name])
        for cap in ("1", "3"):
            assert got[name + "/" + cap] == here, (name, cap)
    # not vacuous: a pass held at most 1 (then 3) of the touched blocks; six calls per fixture and cap, in the child's order
    assert len(lines) == 24, lines
    for i, (form, kind, q, t, p, b) in enumerate(lines):
        cap = (1, 3)[(i // 6) % 2]
        assert (form, kind) == (("host", "device")[i % 2], ("build", "locate", "number")[(i % 6) // 2]) and t >= 4 and p == (t + cap - 1) // cap, (i, lines[i])
    # the questions the table alone answers: no block touched, no pass
    f = fx["LN2"]
    ks, os_ = table_questions(f)
    assert got["table"] == [[_starts(f, ks), [0] * len(ks), ""], [_numbers(f, os_), [0] * len(os_), ""]]
    assert [(x[0], x[1]) for x in table] == [("host", "locate"), ("device", "locate"), ("host", "number"), ("device", "number")]
    assert all(q > 0 and t == 0 and p == 0 and b == 0 for form, kind, q, t, p, b in table), table


def test_several_batches_in_a_pass_give_the_same(L, fx):
    """F1 with at most 250,000 BWT bytes to an inverse-BWT batch (two blocks)"""
    got, lines, table = _run_child(["F1"], {"CJS_DEC_BATCH_ELEMS": "250000"})
    assert got["F1/0"] == _here(L, fx["F1"])
    assert len(lines) == 6 and all(t == 10 and p == 1 and b >= 4 for form, kind, q, t, p, b in lines), lines


def _block_of(bounds, o):
    return int(np.searchsorted(bounds, o, "right")) - 1


def test_damage(L, fx):
    """F1 with the lowest bit of block 4's BWT start flipped (a bad CRC) and the magic of block 7 overwritten, as test_gpu_search"""
    f = fx["F1"]
    e, b, nl, total = f["entries"], f["bounds"], f["nl"], f["total"]
    damaged = f["stream"].copy()
    bit = e[4][0] + 48 + 32 + 1 + 23
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    rg.set_bits(damaged, e[7][0], 48, 0x314159265358)
    dev = lc.on_device(damaged)
    crc_text = r"Bad block CRC \(got [0-9a-f]+ expected %x\)" % e[4][3]
    for rc, t, d in (lc.build_host(L, damaged, f["h"]), lc.build_device(L, dev[1], damaged.size, f["h"])):
        assert rc == rg.E_DATA and not t and re.fullmatch(crc_text, d), (rc, d)
    N = int(nl.size)
    firsts = set()
    put = lambda qs, order: qs if order == 1 else sorted(qs, reverse=True)
    for order in (1, -1):                                   # the lowest-index failing question is in block 4, then (descending) in block 7
        ks = put([k for k in locate_questions(f) if k <= N + 1], order)
        blocks = [_block_of(b, int(nl[k - 1])) if 1 <= k <= N else -1 for k in ks]
        got, st, d = lc.both_forms(L, "locate", damaged, f["h"], f["t"], ks, dev)
        bad = [blk in (4, 7) for blk in blocks]
        assert st == [rg.E_DATA if x else 0 for x in bad] and sum(bad) > 100
        assert got == [0 if x else s for x, s in zip(bad, _starts(f, ks))]
        first = next(blk for blk in blocks if blk in (4, 7))
        assert re.fullmatch(crc_text, d) if first == 4 else d == "index does not match the stream at block 7", (first, d)
        firsts.add(first)
        os_ = put(number_questions(f), order)
        starts = set(int(x) for x in b)
        blocks = [_block_of(b, o) if o < total and o not in starts else -1 for o in os_]
        got, st, d = lc.both_forms(L, "number", damaged, f["h"], f["t"], os_, dev)
        bad = [blk in (4, 7) for blk in blocks]
        assert st == [rg.E_DATA if x else 0 for x in bad] and sum(bad) > 100
        assert got == [0 if x else s for x, s in zip(bad, _numbers(f, os_))]
        first = next(blk for blk in blocks if blk in (4, 7))
        assert re.fullmatch(crc_text, d) if first == 4 else d == "index does not match the stream at block 7", (first, d)
        assert first == (4 if order == 1 else 7)
    assert firsts == {4, 7}


def test_a_table_that_is_not_the_streams(L, fx):
    """the true counts with block 2's off by one: the questions in block 2 fail; those in front of it are right, those behind it
    are what the table says (one newline more in front of them)"""
    f = fx["F1"]
    b, nl, total = f["bounds"], f["nl"], f["total"]
    true = lc.block_counts(f["plain"], b)
    wrong = list(true)
    wrong[2] += 1
    rc, t = lc.create(L, f["h"], wrong)
    assert rc == 0
    cum = np.concatenate([[0], np.cumsum(wrong)])
    N = int(cum[-1])
    text = "line table does not match the stream at block 2"
    ks = [k for k in locate_questions(f) if k <= N + 1]
    blocks = [int(np.searchsorted(cum, k, "left")) - 1 if 1 <= k <= N else -1 for k in ks]
    got, st, d = lc.both_forms(L, "locate", f["stream"], f["h"], t, ks, f["dev"])
    want = [0 if blk == 2 else lc.start(nl, total, k - (1 if blk > 2 else 0)) if k <= N else total for k, blk in zip(ks, blocks)]
    assert st == [rg.E_DATA if blk == 2 else 0 for blk in blocks] and blocks.count(2) > 50 and d == text
    assert got == want
    os_ = number_questions(f)
    starts = set(int(x) for x in b)
    blocks = [_block_of(b, o) if o < total and o not in starts else -1 for o in os_]
    got, st, d = lc.both_forms(L, "number", f["stream"], f["h"], t, os_, f["dev"])
    want = [0 if blk == 2 else lc.number(nl, total, o) + (1 if o >= b[3] else 0) for o, blk in zip(os_, blocks)]
    assert st == [rg.E_DATA if blk == 2 else 0 for blk in blocks] and blocks.count(2) > 50 and d == text
    assert got == want
    L.cjs_bzip2_lines_destroy(t)


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("compressjs-flattened_amd")


@pytest.mark.parametrize("name", ["F1", "LN2"])
def test_read_lines(L, fx, pkg, name):
    f = fx[name]
    stream, plain, nl, total, N = f["stream"], f["plain"], f["nl"], f["total"], int(f["nl"].size)
    ix = pkg.Bzip2Index.build(stream, bool(f["multi"]))
    ln = pkg.Bzip2Lines.build(stream, ix)
    assert ln.newlines == N and ln.counts().tolist() == lc.counts(L, f["t"]) and ln.blocks == len(f["entries"])
    seam = lc.number(nl, total, int(f["bounds"][len(f["bounds"]) // 2]))
    spans = [(0, 1), (N - 1, 1), (N, 1), (max(seam - 1, 0), 3), (N - 1, 10), (N + 5, 2), (0, N + 1), (0, lc.TOP), (3, 0)]
    want = [plain[lc.start(nl, total, a):lc.start(nl, total, min(a + c, lc.TOP))].tobytes() for a, c in spans]
    assert ix.read_lines(stream, ln, spans) == want
    assert want[0].endswith(b"\n") and want[6] == plain.tobytes() and want[5] == b"" and want[8] == b""
    a, c = spans[3]
    assert _block_of(f["bounds"], lc.start(nl, total, a)) < _block_of(f["bounds"], lc.start(nl, total, a + c) - 1)      # across a block seam
    if name == "F1":
        assert want[2] == b""                               # the last byte is a newline: the tail line is empty
    ln2 = pkg.Bzip2Lines.load(ln.save(), ix)
    assert ln2.counts().tolist() == ln.counts().tolist()
    starts, st, d = ix.line_starts(stream, ln, [0, 1, N, N + 1])
    assert starts.tolist() == [lc.start(nl, total, k) for k in (0, 1, N, N + 1)] and not st.any() and d == ""
    numbers, st, d = ix.line_numbers(stream, ln2, [0, total // 2, total])
    assert numbers.tolist() == [lc.number(nl, total, o) for o in (0, total // 2, total)] and not st.any()
    keep, ptr = f["dev"]
    ln3 = pkg.lines_build_device(ptr, stream.size, ix)
    assert ln3.counts().tolist() == ln.counts().tolist()
    assert pkg.line_starts_device(ptr, stream.size, ix, ln3, [2, N])[0].tolist() == [lc.start(nl, total, 2), lc.start(nl, total, N)]
    assert pkg.line_numbers_device(ptr, stream.size, ix, ln3, [total - 1])[0].tolist() == [lc.number(nl, total, total - 1)]
    ln.close(); ln2.close(); ln3.close()


def test_read_lines_on_damage(fx, pkg):
    f = fx["F1"]
    e, b, nl, total = f["entries"], f["bounds"], f["nl"], f["total"]
    ix = pkg.Bzip2Index.build(f["stream"])
    ln = pkg.Bzip2Lines.build(f["stream"], ix)
    damaged = f["stream"].copy()
    rg.set_bits(damaged, e[7][0], 48, 0x314159265358)
    k7 = lc.number(nl, total, int(b[7]) + 1000)
    res = ix.read_lines(damaged, ln, [(5, 2), (k7, 1), (9, 1)])
    assert res[0] == f["plain"][lc.start(nl, total, 5):lc.start(nl, total, 7)].tobytes() and res[2] == f["plain"][lc.start(nl, total, 9):lc.start(nl, total, 10)].tobytes()
    assert isinstance(res[1], pkg.CjsError) and res[1].errorCode == rg.E_DATA and "block 7" in str(res[1])
    with pytest.raises(pkg.CjsError):
        pkg.Bzip2Lines.build(damaged, ix)


def test_grep_lines(fx, pkg):
    f = fx["F1"]
    stream, plain, nl = f["stream"], f["plain"], f["nl"]
    text = plain.tobytes()
    assert b"\r" not in text
    p = int(nl[500])
    k = next(k for k in range(1000, nl.size - 1) if nl[k + 1] - nl[k] >= 10)      # a line of nine bytes or more
    w = int(nl[k]) + 2
    pats = [text[w:w + 4], text[p - 2:p + 3], text[w:w + 3]]      # (the third: a prefix of the first, so some line has two matches)
    assert b"\n" in pats[1] and b"\n" not in pats[0]
    lines = text.splitlines(keepends=True)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).tolist()
    want = {}
    for o, j in sc.expected(plain, pats):
        want.setdefault(bisect.bisect_right(starts, o) - 1, []).append((o, j))
    want = [(no, lines[no], m) for no, m in sorted(want.items())]
    assert any(len(m) > 1 for no, line, m in want) and any(o + len(pats[j]) > starts[no + 1] for no, line, m in want for o, j in m)
    ix = pkg.Bzip2Index.build(stream)
    ln = pkg.Bzip2Lines.build(stream, ix)
    got = ix.grep_lines(stream, ln, pats)
    assert got == want and len(got) >= 3
    assert ix.grep_lines(stream, ln, [b"\x00zq\xffnot here\x01"]) == []
