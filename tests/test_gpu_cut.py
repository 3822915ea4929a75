"""The column cut on the GPU (cjs_bzip2_cut[_device], Bzip2Index.cut_lines, cut_lines_device): every byte of the output against the
restatement over the decoded text (cut_cases.cut_ref: split at the newlines, split at the delimiter or index, join, the tail rule)
-- across 16-byte vectors, thread shares, 16 KiB tiles and blocks, blocks of a few bytes, more than 512 tiles to a chain, a line over
several tiles and over several whole blocks, windows, passes, batches, the device form's room, a damaged block, a foreign and a
wrong table.  Every case runs the host form and the device form (cut_cases.both_forms)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cut_cases as ct
import lines_cases as lc
import range_cases as rg

pytestmark = pytest.mark.gpu

NAMES = ("CT1", "CT2", "CT3")
FIELD_LISTS = ("1", "2", "1,3", "2-", "-2", "3-5,9", "65,300", "1-", "400")
BYTE_LISTS = ("1-3", "5-", "2,4,70-90")
TAB, COMMA, NUL = 9, 44, 0


@pytest.fixture(scope="module")
def L():
    return ct.bind()


@pytest.fixture(scope="module")
def fx(L, oracle):
    return {name: ct.fixture(L, name, oracle) for name in NAMES}


_memo = {}


def want(f, mode, d, spec, first=0, count=None):
    """cut_ref over the fixture's decoded text: computed once per question, shared, never changed"""
    key = (f["name"], mode, d, spec, first, count)
    if key not in _memo:
        _memo[key] = ct.cut_ref(f["text"], mode, d, ct.ref_list(spec), first, count)
    return _memo[key]


def test_the_fixtures_hold_what_the_kernels_can_get_wrong(fx):
    f = fx["CT1"]
    p = ct.properties(f["plain"], f["bounds"])
    assert p["blocks"] >= 3 and 290 * 1024 <= f["total"] <= 320 * 1024
    assert p["fields"] == (0, 12, 300) and p["empty_fields"] >= 1 and p["empty_lines"] >= 1 and p["delimiters_only"] >= 1 and p["tail"] > 0
    assert all(p[k] >= 1 for k in ("across_16", "across_64", "across_80", "across_tile", "across_block")), p
    assert p["delimiter_last_of_tile"] >= 1 and p["delimiter_first_of_tile"] >= 1
    long_line = max(f["text"].split(b"\n"), key=len)
    assert len(long_line) > 2 * ct.TILE and b"\t" not in long_line[100:-100] and b"\t" in long_line[:100] and b"\t" in long_line[-100:]
    assert b"," not in f["text"] and b"\0" not in f["text"]
    f = fx["CT2"]
    p = ct.properties(f["plain"], f["bounds"])
    assert len(f["entries"]) >= 600 and p["tiles"] > 512 and all(1 <= e[2] <= 40 for e in f["entries"]) and len({e[4] for e in f["entries"]}) == 9
    assert max(lc.blocks_of_line(f["nl"], f["total"], f["bounds"], k) for k in range(f["nl"].size + 1)) >= 8
    sizes = np.diff(f["bounds"])
    members = [f["text"][int(a):int(b)] for a, b in zip(f["bounds"][:-1], f["bounds"][1:])]
    assert sum(1 for m in members if b"\n" not in m and b"\t" not in m) >= 8 and f["text"].endswith(b"\n") and b"\0" in f["text"]
    assert ct.CT2_MEMBERS - len(f["entries"]) == 1 and sizes.min() >= 1          # the empty member has no block
    assert fx["CT3"]["total"] == 0 and len(fx["CT3"]["entries"]) == 0


def _all(L, f, mode, d, spec, **kw):
    got, info = ct.both_forms(L, f["stream"], f["h"], f["t"], f["dev"], mode, d, ct.ref_list(spec), **kw)
    return got, info


@pytest.mark.parametrize("name", NAMES)
def test_fields(L, fx, name):
    f = fx[name]
    for spec in FIELD_LISTS:
        got, info = _all(L, f, ct.FIELDS, TAB, spec)
        w = want(f, ct.FIELDS, TAB, spec)
        assert got == w, (spec, _first_difference(got, w))
        assert info == (f["nl"].size + 1, len(w), len(f["entries"]), 0, ct.M64)
    if name == "CT1":
        assert want(f, ct.FIELDS, TAB, "400") == b"\n" * (f["nl"].size + 1) and want(f, ct.FIELDS, TAB, "1-") == f["text"] + b"\n"


def _first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, len(a), len(b), a[max(k - 20, 0):k + 20], b[max(k - 20, 0):k + 20]


@pytest.mark.parametrize("name", NAMES)
def test_bytes(L, fx, name):
    f = fx[name]
    for spec in BYTE_LISTS:
        got, info = _all(L, f, ct.BYTES, 0x0A, spec)          # (delim is ignored: even a newline is no error)
        w = want(f, ct.BYTES, 0, spec)
        assert got == w and info[1] == len(w), (spec, _first_difference(got, w))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("d", (COMMA, NUL))
def test_other_delimiters(L, fx, name, d):
    f = fx[name]
    for spec in ("1", "2-", "1,3"):
        got, info = _all(L, f, ct.FIELDS, d, spec)
        w = want(f, ct.FIELDS, d, spec)
        assert got == w, (spec, _first_difference(got, w))
    if name == "CT1":                                       # the delimiter is absent: every line is one field
        assert want(f, ct.FIELDS, d, "1") == f["text"] + b"\n" and want(f, ct.FIELDS, d, "2-") == b"\n" * (f["nl"].size + 1)


@pytest.mark.parametrize("name", ("CT1", "CT2"))
def test_unordered_and_overlapping_ranges_equal_their_normal_form(L, fx, name):
    f = fx[name]
    for sel in ([(7, 7), (2, 2), (2, 4), (3, 3)], [(70, 90), (1, 1), (80, 300), (65, 66)], [(5, ct.TO_END), (1, 2), (3, 3)], [(2, 2)] * 64):
        for mode in (ct.FIELDS, ct.BYTES):
            got, _ = ct.both_forms(L, f["stream"], f["h"], f["t"], f["dev"], mode, TAB, sel)
            same, _ = ct.both_forms(L, f["stream"], f["h"], f["t"], f["dev"], mode, TAB, ct.normal(sel))
            assert got == same == ct.cut_ref(f["text"], mode, TAB, sel)


def windows(f):
    N = int(f["nl"].size)
    w = [(0, ct.M64), (0, 0), (5, 0), (N + 1, 3), (N + 7, ct.M64), (ct.M64, ct.M64), (3, ct.M64 - 1), (1, ct.M64), (N, 1), (N, 9), (0, N), (0, 1), (7, 1)]
    b = f["bounds"]
    if len(b) > 2:
        mid = lc.number(f["nl"], f["total"], int(b[1]) + (int(b[2]) - int(b[1])) // 2)      # a line that begins in the middle of block 1
        w += [(mid, 1), (mid, 40), (mid + 1, ct.M64), (max(mid - 3, 0), 4)]
        for k in ct.lines_across(f["plain"], b[1:-1])[:2]:      # a line that spans two blocks: first, last, alone, just outside
            w += [(k, 1), (k, 3), (max(k - 2, 0), 3), (k + 1, 2)]
    return w


@pytest.mark.parametrize("name", NAMES)
def test_windows(L, fx, name):
    f = fx[name]
    N = int(f["nl"].size)
    for first, count in windows(f):
        for mode, spec in ((ct.FIELDS, "2-3"), (ct.BYTES, "1-4")):
            got, info = _all(L, f, mode, TAB, spec, first=first, count=count)
            w = want(f, mode, TAB, spec, first, count)
            assert got == w, (first, count, mode, _first_difference(got, w))
            assert info[0] == max(min(first + count, N + 1) - first, 0), (first, count)
    if name == "CT1":
        assert want(f, ct.FIELDS, TAB, "2-3", N, 1) == b"of\tit\n"          # the window of only the tail line
        one = want(f, ct.FIELDS, TAB, "2-3", 7, 1)                           # one line inside one tile
        assert one.count(b"\n") == 1 and lc.start(f["nl"], f["total"], 8) < ct.TILE


def test_a_window_touches_only_its_blocks(L, fx):
    f = fx["CT1"]
    k = lc.number(f["nl"], f["total"], int(f["bounds"][1]) + 5000)          # a line in block 1
    got, info = _all(L, f, ct.FIELDS, TAB, "1", first=k + 1, count=5)
    assert info[2] == 1 and got == want(f, ct.FIELDS, TAB, "1", k + 1, 5)


# ---------------------------------------------------------------- the device form's room
@pytest.mark.parametrize("name", ("CT1", "CT2"))
def test_device_form_room(L, fx, name):
    f = fx[name]
    n = f["stream"].size
    for mode, spec in ((ct.FIELDS, "2"), (ct.FIELDS, "1-"), (ct.BYTES, "2,4,70-90")):
        sel = ct.ref_list(spec)
        w = want(f, mode, TAB, spec)
        call = lambda **kw: ct.cut_device(L, f["dev"][1], n, f["h"], f["t"], mode, TAB, sel, **kw)      # (cut_device checks the canaries around d_out[0 .. out_cap))
        rc, got, need, info, d = call(out_cap=len(w) - 1)
        assert rc == rg.E_TOO_SMALL and need == len(w) and got == w[:-1] and info.out_bytes == len(w)
        rc, got, need, info, d = call(out_cap=len(w) // 2 + 3)                  # the passes behind the one that fills d_out still count
        assert rc == rg.E_TOO_SMALL and need == len(w) and got == w[:len(w) // 2 + 3]
        rc, got, need, info, d = call(out_cap=None)                             # the size query, then exactly that much
        assert rc == 0 and need == len(w) and got == w
        rc, got, need, info, d = call(out_cap=f["total"] + 1)                   # the window's bytes + 1 are always enough
        assert rc == 0 and got == w
        for shift in (1, 3, 15):
            rc, got, need, info, d = call(out_cap=len(w), shift=shift)
            assert rc == 0 and got == w, shift


# ---------------------------------------------------------------- passes and batches
def digest(got, info):
    return [hashlib.sha256(got).hexdigest(), list(info)]


def _span(f):
    """the lines the pass tests ask for: all of CT1; of CT2 (a block per member, so a pass per member or two) forty lines"""
    return dict(first=int(f["nl"].size) // 3, count=40) if f["name"] == "CT2" else dict(first=0, count=ct.M64)


def _digests(L, f, t):
    N = int(f["nl"].size)
    forms = lambda *a, **kw: ct.both_forms(L, f["stream"], f["h"], t, f["dev"], *a, **kw)
    return [digest(*forms(ct.FIELDS, TAB, ct.ref_list("2-3"), **_span(f))), digest(*forms(ct.BYTES, TAB, ct.ref_list("5-"), **_span(f))),
            digest(*forms(ct.FIELDS, TAB, ct.ref_list("1,3"), first=N // 3, count=min(N // 2, _span(f)["count"])))]


def child(names, env):
    """(the child of the two tests below) the fixtures `names` under the environment `env`: {name/setting: digests}; the [cjs cut]
    lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    for k, v in env.items():
        if k != "CJS_RANGE_PASS_BLOCKS":
            os.environ[k] = v
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = ct.bind(), support.Oracle(), {}
    for name in names:
        os.environ["CJS_RANGE_PASS_BLOCKS"] = "0"
        f = ct.fixture(L, name, oracle)
        for cap in env.get("CJS_RANGE_PASS_BLOCKS", "0").split(","):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            out[name + "/" + cap] = _digests(L, f, f["t"])
    print(json.dumps(out))


LINE = r"\[cjs cut\] (host|device): lines \[(\d+), (\d+)\), (\d+) of \d+ blocks touched, (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\), (\d+) cut batches"


def _run_child(names, env):
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_cut as t; t.child(%r, %r)" % (names, env)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=penv,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [(form,) + tuple(int(x) for x in rest) for form, *rest in re.findall(LINE, run.stderr)]
    return json.loads(run.stdout.strip().splitlines()[-1]), lines


def test_several_passes_give_the_one_pass_bytes(L, fx):
    got, lines = _run_child(["CT1", "CT2"], {"CJS_RANGE_PASS_BLOCKS": "1,2"})
    for name in ("CT1", "CT2"):
        here = _digests(L, fx[name], fx[name]["t"])
        span = _span(fx[name])
        assert here[0][0] == hashlib.sha256(want(fx[name], ct.FIELDS, TAB, "2-3", span["first"], span["count"])).hexdigest()
        for cap in ("1", "2"):
            assert got[name + "/" + cap] == here, (name, cap)
    # not vacuous: a pass held at most `cap` of the touched blocks, and every pass's batch was cut on its own.  Per fixture and cap
    # three questions, each the host form, the size query and the device form.
    assert len(lines) == 2 * 2 * 9, len(lines)
    for i, (form, a, b, t, p, bt, cb) in enumerate(lines):
        cap = (1, 2)[(i // 9) % 2]
        assert form == ("host", "device", "device")[i % 3] and t >= 2 and p == (t + cap - 1) // cap and cb == bt >= p, (i, lines[i])


def test_several_batches_in_a_pass_give_the_same(L, fx):
    """CT1 with at most 150,000 BWT bytes to an inverse-BWT batch (one block): the state goes from batch to batch"""
    got, lines = _run_child(["CT1"], {"CJS_DEC_BATCH_ELEMS": "150000"})
    assert got["CT1/0"] == _digests(L, fx["CT1"], fx["CT1"]["t"])
    assert len(lines) == 9 and all(p == 1 and bt >= 3 and cb == bt for form, a, b, t, p, bt, cb in lines[:6]), lines


# ---------------------------------------------------------------- what is not the stream's
def test_damage(L, fx):
    """CT1 with one bit flipped in block 1 (the lowest bit of its BWT start): a window that touches it fails with read_ranges' detail
    and info filled, in both forms; a window that does not is served"""
    f = fx["CT1"]
    e, b = f["entries"], f["bounds"]
    blk = 1
    damaged = f["stream"].copy()
    bit = e[blk][0] + 48 + 32 + 1 + 23
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    dev = lc.on_device(damaged)
    rc, buf, _, _, st, detail = rg.read_host(L, damaged, f["h"], [(int(b[blk]) + 10, 5)])
    assert rc == 0 and st[0] == rg.E_DATA and detail
    sel = ct.ref_list("2")
    rc, got, info, d = ct.cut_host(L, damaged, f["h"], f["t"], ct.FIELDS, TAB, sel)
    assert rc == rg.E_DATA and got is None and d == detail and (info.n_bad_blocks, info.first_bad_block) == (1, blk) and info.blocks_decoded == len(e)
    rc, got, need, info, d = ct.cut_device(L, dev[1], damaged.size, f["h"], f["t"], ct.FIELDS, TAB, sel, out_cap=f["total"] + 1)
    assert rc == rg.E_DATA and d == detail and (info.n_bad_blocks, info.first_bad_block) == (1, blk)
    # windows in front of the block and behind it
    first_behind = lc.number(f["nl"], f["total"], int(b[blk + 1])) + 1
    last_in_front = lc.number(f["nl"], f["total"], int(b[blk]) - 1) - 1
    for first, count in ((0, last_in_front), (first_behind, ct.M64)):
        got, info = ct.both_forms(L, damaged, f["h"], f["t"], dev, ct.FIELDS, TAB, sel, first=first, count=count)
        assert got == want(f, ct.FIELDS, TAB, "2", first, count) and info[3] == 0 and len(got) > 1000


def test_tables_that_are_not_the_streams(L, fx):
    f, other = fx["CT1"], fx["CT2"]
    sel = ct.ref_list("1")
    rc, got, info, d = ct.cut_host(L, f["stream"], f["h"], other["t"], ct.FIELDS, TAB, sel)
    assert rc == rg.E_INVALID and d == lc.FOREIGN
    rc, got, need, info, d = ct.cut_device(L, f["dev"][1], f["stream"].size, f["h"], other["t"], ct.FIELDS, TAB, sel, out_cap=64)
    assert rc == rg.E_INVALID and d == lc.FOREIGN
    # two counts swapped: the totals still agree with the index, the stream does not
    counts = lc.block_counts(f["plain"], f["bounds"])
    assert counts[1] != counts[2]
    wrong = list(counts)
    wrong[1], wrong[2] = wrong[2], wrong[1]
    rc, t = lc.create(L, f["h"], wrong)
    assert rc == 0
    rc, got, info, d = ct.cut_host(L, f["stream"], f["h"], t, ct.FIELDS, TAB, sel)
    assert rc == rg.E_DATA and d == ct.MISMATCH % 1 and got is None
    rc, got, need, info, d = ct.cut_device(L, f["dev"][1], f["stream"].size, f["h"], t, ct.FIELDS, TAB, sel, out_cap=f["total"] + 1)
    assert rc == rg.E_DATA and d == ct.MISMATCH % 1
    got, info = ct.both_forms(L, f["stream"], f["h"], t, f["dev"], ct.FIELDS, TAB, sel, first=0, count=counts[0] - 5)      # a window in front of block 1 is served
    assert got == want(f, ct.FIELDS, TAB, "1", 0, counts[0] - 5)
    L.cjs_bzip2_lines_destroy(t)


# ---------------------------------------------------------------- the Python front
@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("compressjs-flattened_amd")


def test_python_front(fx, pkg):
    import torch
    f = fx["CT1"]
    ix = pkg.Bzip2Index.build(f["stream"])
    ln = pkg.Bzip2Lines.build(f["stream"], ix)
    w = want(f, ct.FIELDS, TAB, "1,3-5")
    assert pkg.cut_list("1,3-5,7-") == [(1, 1), (3, 5), (7, pkg.CUT_TO_END)]
    assert ix.cut_lines(f["stream"], ln, fields="1,3-5") == w
    assert ix.cut_lines(f["stream"], ln, fields=[1, (3, 5)]) == w and ix.cut_lines(f["stream"], ln, fields=[(4, 5), 3, 1, (3, 3)], delimiter="\t") == w
    assert ix.cut_lines(f["stream"], ln, fields=[(2, None)], delimiter=9) == want(f, ct.FIELDS, TAB, "2-")
    assert ix.cut_lines(f["stream"], ln, bytes="1-3") == want(f, ct.BYTES, 0, "1-3")
    assert ix.cut_lines(f["stream"], ln, fields="2-3", first=7, count=3) == want(f, ct.FIELDS, TAB, "2-3", 7, 3)
    assert pkg.cut_text(f["text"], fields="1,3-5") == w and pkg.cut_text(b"a,b\nc", fields=[2], delimiter=b",") == b"b\n\n"
    for kw in (dict(), dict(fields="1", bytes="1"), dict(fields="1", delimiter=b"ab"), dict(fields="1", delimiter=b"")):
        with pytest.raises(ValueError):
            ix.cut_lines(f["stream"], ln, **kw)
    for kw in (dict(fields="0"), dict(fields=[(3, 2)]), dict(fields="1", delimiter=b"\n"), dict(fields="")):
        with pytest.raises(pkg.CjsError) as e:
            ix.cut_lines(f["stream"], ln, **kw)
        assert e.value.errorCode == rg.E_INVALID
    d_in = torch.from_numpy(f["stream"].copy()).cuda()
    with pytest.raises(pkg.CjsError) as e:
        pkg.cut_lines_device(d_in.data_ptr(), d_in.numel(), ix, ln, fields="1,3-5")
    assert e.value.errorCode == rg.E_TOO_SMALL and e.value.need == len(w)
    d_out = torch.zeros(len(w) + 8, dtype=torch.uint8, device="cuda")
    n = pkg.cut_lines_device(d_in.data_ptr(), d_in.numel(), ix, ln, fields="1,3-5", d_out_ptr=d_out.data_ptr(), out_cap=d_out.numel())
    assert n == len(w) and d_out[:n].cpu().numpy().tobytes() == w
