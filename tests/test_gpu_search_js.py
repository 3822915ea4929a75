"""Pattern search through the JavaScript front (Bzip2.search) on the GPU, on F1 and S4: the lists are plain Python's over the
decoded text, with strings, Buffers and Uint8Arrays as patterns, a window, nocase, a limit and a damaged block."""
import json
import os
import shutil
import subprocess

import pytest

import range_cases as rg
import search_cases as sc
import support

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_js_search_matches_python(tmp_path):
    oracle = support.Oracle()
    f1, plain1, _, _ = rg.f1()
    s4, plain4, _ = sc.s4(oracle)
    src1, src4, bad1 = str(tmp_path / "f1.bz2"), str(tmp_path / "s4.bz2"), str(tmp_path / "bad.bz2")
    f1.tofile(src1)
    s4.tofile(src4)
    rc, tab = oracle.bzip2_table(f1, 0)
    assert rc == 0
    damaged = f1.copy()
    rg.set_bits(damaged, tab[7][0], 48, 0x314159265358)      # the magic of block 7
    damaged.tofile(bad1)
    B = 3 * 99981
    seam = [bytes(plain1[B - 1:B + 1]), bytes(plain1[B - 128:B + 128]), b"court", b"Court", bytes(plain1[B - 255:B + 1])]
    tiny = [bytes(plain4[100:100 + n]) for n in (1, 2, 3, 17, 40)]
    hexes = lambda pats: [p.hex() for p in pats]
    cases = [
        dict(path=src1, multistream=False, patterns=hexes(seam), opts={}),
        dict(path=src1, multistream=False, patterns=hexes([b"COURT", b"ses", b"Cour"]), asStrings=True, opts={"offset": B - 2, "length": 5000, "nocase": True, "limit": 7}),
        dict(path=src4, multistream=True, patterns=hexes(tiny), opts={"offset": 3}),
        dict(path=src1, multistream=False, patterns=hexes(seam), opts={"limit": 0}, damaged=bad1),
    ]
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_search_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    r = rep["cases"]
    want = sc.expected(plain1, seam)
    assert r[0] == dict(matches=[list(m) for m in want], total=len(want), badBlocks=0, firstBadBlock=None, detail="") and (B - 128, 1) in want
    want = sc.expected(plain1, [b"COURT", b"ses", b"Cour"], B - 2, 5000, nocase=True)
    assert r[1]["matches"] == [list(m) for m in want[:7]] and r[1]["total"] == len(want) > 7
    want = sc.expected(plain4, tiny, 3)
    assert r[2]["matches"] == [list(m) for m in want] and r[2]["total"] == len(want) and (100, 4) in want
    runs = [(0, 7 * 99981), (8 * 99981, plain1.size)]
    assert r[3] == dict(matches=[], total=len(sc.expected(plain1, seam, runs=runs)), badBlocks=1, firstBadBlock=7, detail="index does not match the stream at block 7")
    ref = rep["refusals"]
    for k in ("none", "empty", "long", "notAnIndex"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
    assert ref["fraction"]["error"] == "TypeError:offsets and lengths are integers from 0 to 2^53"
