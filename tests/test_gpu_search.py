"""Pattern search on the GPU (cjs_bzip2_search[_device], Bzip2Index.search / grep): every list against plain Python's search of the
decoded text -- across block seams, blocks of a few bytes, tile seams, passes and batches, windows, caps, case folding, 64
patterns and damaged blocks.  Every case runs the host form and the device form (search_cases.both_forms)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import range_cases as rg
import search_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return sc.bind()


def _fixture(L, name, oracle):
    if name in ("F1", "F2"):
        stream, plain, multi, _ = rg.fixture(name, oracle)
        extra = ()
    elif name == "S4":
        stream, plain, multi = sc.s4(oracle)
        extra = ()
    else:
        stream, plain, at37, at256 = sc.s5(oracle)
        multi, extra = 0, (at37, at256)
    rc, h = rg.build(L, stream, multi)
    assert rc == 0, (name, rc, rg.detail(L))
    e = rg.entries(L, h)
    bounds = np.concatenate([[0], np.cumsum([x[2] for x in e])]).astype(np.int64)
    return dict(stream=stream, plain=plain, h=h, entries=e, bounds=bounds, extra=extra)


@pytest.fixture(scope="module")
def fx(L, oracle):
    return {name: _fixture(L, name, oracle) for name in ("F1", "F2", "S4", "S5")}


def _seam_set(f):
    """F1's block-seam patterns, the 1-byte and the 3-byte one being the text's most frequent"""
    plain = f["plain"]
    pats = sc.seam_patterns(plain, f["bounds"][1:-1])
    tri = (plain[:-2].astype(np.uint32) << 16) | (plain[1:-1].astype(np.uint32) << 8) | plain[2:]
    v, c = np.unique(tri, return_counts=True)
    t = int(v[c.argmax()])
    pats[-4] = bytes([int(np.bincount(plain).argmax())])
    pats[-3] = bytes([t >> 16, (t >> 8) & 255, t & 255])
    return pats


def _tiny_set(f):
    """prefixes of 1..40 bytes of the 40 bytes of the plain that cover the most blocks"""
    b = f["bounds"]
    cover = [int(np.searchsorted(b, s + 40, "left") - np.searchsorted(b, s, "right")) + 1 for s in range(f["plain"].size - 40)]
    s = int(np.argmax(cover))
    return [bytes(f["plain"][s:s + n]) for n in range(1, 41)], s


def _blocks_of(f, o, n):
    """blocks of non-zero size that [o, o + n) overlaps"""
    b = f["bounds"]
    return sum(1 for k in range(len(b) - 1) if b[k + 1] > b[k] and b[k] < o + n and b[k + 1] > o)


def test_block_seams(L, fx):
    f = fx["F1"]
    pats = _seam_set(f)
    assert len(pats) == 9 * 5 + 4 and pats[-1] == pats[1]
    want = sc.expected(f["plain"], pats)
    for k, B in enumerate(f["bounds"][1:-1]):              # the five patterns of every seam are found where they were cut
        B = int(B)
        assert {(B - 1, 5 * k), (B - 7, 5 * k + 1), (B - 255, 5 * k + 2), (B - 1, 5 * k + 3), (B - 128, 5 * k + 4)} <= set(want)
    assert not [m for m in want if m[1] == len(pats) - 2] and len([m for m in want if m[1] == len(pats) - 4]) > 10000
    got, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
    assert got == want and info == (len(want), 0, 2 ** 64 - 1, 10) and d == ""


@pytest.mark.parametrize("name", ["S4", "F2"])
def test_tiny_blocks(L, fx, name):
    f = fx[name]
    pats, s = _tiny_set(f)
    want = sc.expected(f["plain"], pats)
    assert max(_blocks_of(f, o, len(pats[j])) for o, j in want) >= 4 and (s, 39) in want
    got, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
    assert got == want and info[:3] == (len(want), 0, 2 ** 64 - 1) and d == ""
    if name == "S4":                                        # the three shortest patterns of the issue, as they are
        pats = [b"a", b"ab", b"aba"]
        got, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
        assert got == sc.expected(f["plain"], pats) and len(got) > 100


def test_tile_seams(L, fx):
    f = fx["S5"]
    at37, at256 = f["extra"]
    pats = [sc.M37, sc.M256]
    want = sorted([(p, 0) for p in at37] + [(p, 1) for p in at256])
    assert sc.expected(f["plain"], pats) == want and len(at37) > 100 and len(at256) > 100
    for kind in (at37, at256):                              # every d at the seams of 16 KiB, and of 1 KiB
        assert {p - 16384 * round(p / 16384) for p in kind if abs(p - 16384 * round(p / 16384)) < 40} == {-37, -36, -1, 0, 1}
        assert {p - 1024 * round(p / 1024) for p in kind} == {-37, -36, -1, 0, 1}
    got, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
    assert got == want and d == ""


def _pass_cases(L, fx):
    """name -> (fixture, patterns) of the several-pass and several-batch runs"""
    sets = {"F1": _seam_set, "S4": lambda f: _tiny_set(f)[0]}
    return {name: (fx[name], sets[name](fx[name])) for name in ("F1", "S4") if name in fx}


def child(names, env):
    """(the child of the two tests below) the fixtures `names` under the environment `env`: {name/setting: result of both_forms};
    the [cjs search] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    for k, v in env.items():
        if k != "CJS_RANGE_PASS_BLOCKS":
            os.environ[k] = v
    import torch  # noqa: F401  (one HIP runtime per process: torch's copy is loaded before the library)
    import support
    L, oracle, out = sc.bind(), support.Oracle(), {}
    fx = {name: _fixture(L, name, oracle) for name in names}
    for name in names:
        f, pats = _pass_cases(L, fx)[name]
        for cap in env.get("CJS_RANGE_PASS_BLOCKS", "0").split(","):
            os.environ["CJS_RANGE_PASS_BLOCKS"] = cap       # (read at every call)
            got, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
            out[name + "/" + cap] = [got, list(info), d]
    print(json.dumps(out))


def _run_child(names, env):
    penv = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    code = "import test_gpu_search as t; t.child(%r, %r)" % (names, env)
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], capture_output=True, text=True, env=penv,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    lines = re.findall(r"\[cjs search\] (host|device): .*? (\d+) of \d+ blocks touched, .*? (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\)", run.stderr)
    return json.loads(run.stdout.strip().splitlines()[-1]), [(form, int(t), int(p), int(b)) for form, t, p, b in lines]


def test_several_passes_give_the_one_pass_list(L, fx):
    got, lines = _run_child(["F1", "S4"], {"CJS_RANGE_PASS_BLOCKS": "1,3"})
    for name, (f, pats) in _pass_cases(L, fx).items():
        here, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
        assert here == sc.expected(f["plain"], pats)
        for cap in ("1", "3"):
            assert got[name + "/" + cap] == [[list(m) for m in here], list(info), d], (name, cap)
    # not vacuous: a pass held at most 1 (then 3) of the touched blocks
    assert len(lines) == 16 and all(p >= 4 for form, t, p, b in lines), lines
    assert any(p == t for form, t, p, b in lines) and any(p == (t + 2) // 3 for form, t, p, b in lines)


def test_several_batches_in_a_pass_give_the_same(L, fx):
    """F1 with at most 250,000 BWT bytes to an inverse-BWT batch (two blocks): the carry crosses batches inside one pass"""
    got, lines = _run_child(["F1"], {"CJS_DEC_BATCH_ELEMS": "250000"})
    f, pats = _pass_cases(L, fx)["F1"]
    here, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
    assert got["F1/0"] == [[list(m) for m in here], list(info), d]
    assert len(lines) == 4 and all(p == 1 and b >= 4 for form, t, p, b in lines), lines


def _one_call(L, f, pats, off, ln, want):
    """both forms with cap a little above the expected number, no count query: the list and n_matches"""
    import torch
    n = f["stream"].size
    rc, m, info, d = sc.search_host(L, f["stream"], f["h"], pats, off, ln, 0, len(want) + 4)
    assert rc == 0 and m == want and info.n_matches == len(want) and d == "", (off, ln)
    d_in = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    d_in[5:5 + n] = torch.from_numpy(f["stream"]).cuda()
    torch.cuda.synchronize()
    rc, m2, info2, d2 = sc.search_device(L, d_in.data_ptr() + 5, n, f["h"], pats, off, ln, 0, len(want) + 4)
    assert rc == 0 and m2 == want and sc.info_tuple(info2) == sc.info_tuple(info), (off, ln)
    return info


def test_windows(L, fx):
    f = fx["F1"]
    plain, total = f["plain"], int(f["bounds"][-1])
    for k, B in enumerate(f["bounds"]):
        B = int(B)
        lo, hi = max(B - 300, 0), min(B + 300, total)
        pats = [bytes(plain[max(B - 1, 0):B + 1]), bytes(plain[max(B - 7, 0):B + 9]), bytes(plain[max(B - 128, 0):B + 128]), bytes(plain[lo:lo + 1])]
        pats = [p for p in pats if p]
        for d in (-1, 0, 1):
            if 0 <= B + d <= total:
                _one_call(L, f, pats, B + d, hi - (B + d) if hi > B + d else 0, sc.expected(plain, pats, B + d, max(hi - (B + d), 0)))      # starts there
                _one_call(L, f, pats, lo, max(B + d - lo, 0), sc.expected(plain, pats, lo, max(B + d - lo, 0)))                              # ends there
    # a window that ends one byte short of a match's last byte, and one that ends exactly on it
    B = int(f["bounds"][3])
    p = [bytes(plain[B - 20:B + 30])]
    assert sc.expected(plain, p) == [(B - 20, 0)]
    info = _one_call(L, f, p, B - 1000, 1000 + 29, [])
    assert info.blocks_decoded == 2
    _one_call(L, f, p, B - 1000, 1000 + 30, [(B - 20, 0)])
    _one_call(L, f, p, B - 20, 50, [(B - 20, 0)])
    _one_call(L, f, p, B - 19, 50, [])
    # len = 0, off >= total, len = 2^64 - 1
    few = [bytes(plain[total - 9:]), bytes(plain[:300000 + 7][-7:])]
    for off, ln in ((5, 0), (total, 10), (total + 5, sc.ALL), (2 ** 64 - 1, sc.ALL)):
        info = _one_call(L, f, few, off, ln, [])
        assert info.blocks_decoded == 0
    for off in (0, 300000, total - 9, total - 8):
        info = _one_call(L, f, few, off, sc.ALL, sc.expected(plain, few, off, sc.ALL))
        assert info.blocks_decoded == 10 - off // 99981 or off >= 9 * 99981
    assert sc.expected(plain, few, total - 9, sc.ALL)[-1] == (total - 9, 0) and (total - 9, 0) not in sc.expected(plain, few, total - 8, sc.ALL)


def test_cap(L, fx):
    f = fx["F1"]
    pats = [bytes(f["plain"][1000:1003]), b"e", bytes(f["plain"][1000:1003])]
    want = sc.expected(f["plain"], pats)
    total = len(want)
    assert total > 1000
    for cap in (0, 1, 2, 777, total - 1, total, total + 5):      # (the canary behind entry min(cap, total) is checked in search_cases._call)
        got, info, d = sc.both_forms(L, f["stream"], f["h"], pats, cap=cap)
        assert got == want[:cap] and info[0] == total, cap


def child_caps(elems, calls):
    """(a child as well) S4 with at most `elems` BWT bytes to an inverse-BWT batch: [result of both_forms(pats, cap=cap)] for every
    (pats, cap) of `calls`; the [cjs search] lines go to stderr"""
    os.environ["CJS_DEBUG"] = "1"
    os.environ["CJS_DEC_BATCH_ELEMS"] = elems
    import torch  # noqa: F401
    import support
    L = sc.bind()
    f = _fixture(L, "S4", support.Oracle())
    print(json.dumps([list(sc.both_forms(L, f["stream"], f["h"], pats, cap=cap)) for pats, cap in calls]))


def test_cap_runs_out_in_a_later_batch(L, fx):
    """S4 in inverse-BWT batches of at most 40 bytes (its 234 bytes, at least 195 after RLE1: five batches or more in one pass).  The list gets full in the
    middle of a later batch, in the first batch with matches in every later one, and in the first batch with none behind it: the
    first cap matches, and n_matches counts on."""
    f = fx["S4"]
    many, head = [b"a", b"ab", b"aba"], [bytes(f["plain"][:12])]
    want = sc.expected(f["plain"], many)
    assert len(want) > 100 and sc.expected(f["plain"], head) == [(0, 0)]
    assert want[len(want) // 2][0] > 80 and want[-1][0] > 200      # (half of the list lies behind the second batch; the last batch has matches)
    calls = [(many, len(want) // 2), (many, 1), (head, 1), (head + many, 3)]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", "import test_gpu_search as t; t.child_caps('40', %r)" % (calls,)], capture_output=True,
                         text=True, env=dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path)), cwd=os.path.dirname(os.path.abspath(__file__)))
    assert run.returncode == 0, run.stderr[-3000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    blocks = sum(1 for e in f["entries"] if e[2])
    for (pats, cap), (m, info, d) in zip(calls, got):
        full = sc.expected(f["plain"], pats)
        assert [tuple(x) for x in m] == full[:cap] and tuple(info) == (len(full), 0, 2 ** 64 - 1, blocks) and d == "", (pats, cap)
    lines = re.findall(r"\[cjs search\] (?:host|device): .*? (\d+) passes \(\d+ row batches, (\d+) inverse-BWT batches\)", run.stderr)
    assert len(lines) == 4 * len(calls) and all(int(p) == 1 and int(b) >= 5 for p, b in lines), lines


def test_nocase(L, oracle):
    """mixed-case text with bytes >= 0x80 (0xC1 / 0xE1 differ by 0x20 like A / a) and @ [ ` { next to letters: only A..Z fold"""
    rng = np.random.RandomState(8)
    alphabet = np.frombuffer(b"aAbBzZmM@[`{\xc1\xe1\xda\xfa ", np.uint8)
    plain = alphabet[rng.randint(0, alphabet.size, 150000)]
    rc, s = oracle.bzip2_compress(plain, 1)
    assert rc == 0
    stream = np.asarray(s, dtype=np.uint8)
    rc, h = rg.build(L, stream, 0)
    assert rc == 0
    pats = [b"Ab", b"zZ@", b"[a", b"\xc1A", b"`b{", b"\xe1a", b"@", b"`", b"Mm\xdaz", b"aBzM", b"ABZM", b"{", b"[", b"Z"]
    for flags in (sc.NOCASE, 0):
        want = sc.expected(plain, pats, nocase=bool(flags))
        got, info, d = sc.both_forms(L, stream, h, pats, flags=flags)
        assert got == want and len(want) > 1000, flags
    folded = sc.expected(plain, pats, nocase=True)
    by = lambda j: [o for o, k in folded if k == j]
    assert by(9) == by(10) and by(3) != by(5) and len(by(6)) == int((plain == ord("@")).sum()) and len(by(13)) == int(((plain | 32) == ord("z")).sum())
    L.cjs_bzip2_index_destroy(h)


def test_64_patterns(L, fx):
    f = fx["F1"]
    plain = f["plain"]
    rng = np.random.RandomState(64)
    lens = [1, 2, 3, 4, 5, 255, 256] + [int(x) for x in rng.randint(1, 257, 45)]
    pats = [bytes(plain[s:s + n]) for s, n in zip(rng.randint(0, plain.size - 300, len(lens)), lens)]
    base = int(rng.randint(0, plain.size - 300))
    pats += [bytes(plain[base:base + 4]) + x for x in (b"", b"q", bytes(plain[base + 4:base + 9]), bytes(plain[base + 4:base + 200]), b"\x00\x00")]      # one 4-byte prefix
    pats += [pats[10][:7], pats[10], pats[10]]              # a prefix of another; duplicates
    pats += [b"th", b"the", b"the ", b"ther"]
    assert len(pats) == 64 and sorted(set(len(p) for p in pats))[0] == 1 and max(len(p) for p in pats) == 256
    want = sc.expected(plain, pats)
    assert {j for o, j in want} >= set(range(52)) | {52, 54, 55, 57, 58, 59}
    got, info, d = sc.both_forms(L, f["stream"], f["h"], pats)
    assert got == want


def test_damage(L, fx):
    """F1 with the lowest bit of block 4's BWT start flipped (the block decodes to as many bytes, other ones: a bad CRC) and the
    magic of block 7 overwritten: the matches of the runs 0..3, 5..6, 8..9, each searched on its own"""
    f = fx["F1"]
    e, b, plain = f["entries"], f["bounds"], f["plain"]
    damaged = f["stream"].copy()
    bit = e[4][0] + 48 + 32 + 1 + 23
    damaged[bit >> 3] ^= 1 << (7 - (bit & 7))
    rg.set_bits(damaged, e[7][0], 48, 0x314159265358)
    pats = _seam_set(f)
    runs = [(int(b[0]), int(b[4])), (int(b[5]), int(b[7])), (int(b[8]), int(b[10]))]
    want = sc.expected(plain, pats, runs=runs)
    seam = lambda k: {(int(b[k]) - 1, 5 * (k - 1)), (int(b[k]) - 7, 5 * (k - 1) + 1), (int(b[k]) - 255, 5 * (k - 1) + 2), (int(b[k]) - 128, 5 * (k - 1) + 4)}
    assert seam(6) <= set(want) and not any(seam(k) & set(want) for k in (4, 5, 7, 8))
    got, info, d = sc.both_forms(L, damaged, f["h"], pats)
    assert info == (len(want), 2, 4, 10)
    assert re.fullmatch(r"Bad block CRC \(got [0-9a-f]+ expected %x\)" % e[4][3], d), d
    assert got == want
    # only the bad magic: the other of read_ranges' two texts
    only7 = f["stream"].copy()
    rg.set_bits(only7, e[7][0], 48, 0x314159265358)
    got, info, d = sc.both_forms(L, only7, f["h"], pats, off=int(b[6]) + 5)
    assert info[1:] == (1, 7, 4) and d == "index does not match the stream at block 7"
    assert got == sc.expected(plain, pats, off=int(b[6]) + 5, runs=[(int(b[6]), int(b[7])), (int(b[8]), int(b[10]))])


def test_python_front(fx):
    import importlib
    import torch
    pkg = importlib.import_module("compressjs-flattened_amd")
    f = fx["F1"]
    stream, plain = f["stream"], f["plain"]
    ix = pkg.Bzip2Index.build(stream)
    B = int(f["bounds"][2])
    pats = [bytes(plain[B - 5:B + 5]), "the", np.frombuffer(b"THE", np.uint8)]
    res = ix.search(stream, pats)
    assert res.matches == sc.expected(plain, [pats[0], b"the", b"THE"]) and res.total == len(res.matches)
    assert (res.bad_blocks, res.first_bad_block, res.detail, res.blocks_decoded) == (0, None, "", 10)
    few = ix.search(stream, pats, off=B - 5, length=4000, nocase=True, limit=3)
    want = sc.expected(plain, [pats[0], b"the", b"THE"], B - 5, 4000, nocase=True)
    assert few.matches == want[:3] and few.total == len(want) > 3
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    dev = pkg.search_device(d_in.data_ptr(), stream.size, ix, pats, off=B - 5, length=4000, nocase=True)
    assert dev.matches == want and dev.total == len(want)
    ctx = ix.grep(stream, [pats[0]], before=3, after=4)
    assert ctx == [(B - 5, 0, plain[B - 8:B + 9].tobytes())]
    ctx = ix.grep(stream, [plain[:4].tobytes()], before=10, after=2, length=100)
    assert ctx[0] == (0, 0, plain[:6].tobytes())
    damaged = stream.copy()
    damaged[(f["entries"][5][0] + f["entries"][5][1]) // 16] ^= 0x04
    res = ix.search(damaged, pats)
    assert res.bad_blocks == 1 and res.first_bad_block == 5 and "block" in res.detail.lower()
    with pytest.raises(pkg.CjsError):
        ix.search(stream, [])
