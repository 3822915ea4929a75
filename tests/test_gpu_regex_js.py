"""Regex search through the JavaScript front (Bzip2.searchRegex, Bzip2.regexCheck) on the GPU, on F1 and S4: the lists are the
Python front's (and `re`'s), with strings, Buffers and Uint8Arrays as patterns, a window, nocase, a limit and a damaged block;
the messages of the refusals."""
import importlib
import json
import os
import shutil
import subprocess

import pytest

import range_cases as rg
import regex_cases as rx
import search_cases as sc
import support

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_js_regex_search_matches_python(tmp_path):
    pkg = importlib.import_module("compressjs-flattened_amd")
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
    words = [rb"[A-Z][a-z]+'s", rb"[a-z]+ing\n", rb"\x41[^\n]{0,3}\n"]
    tiny = [rb"a+b", rb"(ab){1,20}", rb"b[ab]{0,255}"]
    hexes = lambda pats: [p.hex() for p in pats]
    W = dict(off=5, length=40000)
    cases = [
        dict(path=src1, multistream=False, patterns=hexes(words), opts=dict(offset=W["off"], length=W["length"])),
        dict(path=src1, multistream=False, patterns=hexes([rb"COURT[a-z]*", rb"[^a-z]s+e"]), asStrings=True, opts={"offset": B - 2, "length": 50000, "nocase": True, "limit": 7}),
        dict(path=src4, multistream=True, patterns=hexes(tiny), opts={"offset": 3}),
        dict(path=src1, multistream=False, patterns=hexes(words[:1]), opts={"limit": 0}, damaged=bad1),
    ]
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases, "check": hexes(words + tiny)}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_regex_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    r = rep["cases"]
    # against the Python front, and that against re
    py = pkg.Bzip2Index.build(f1).search_regex(f1, words, **W)
    want = rx.expected(plain1, words, W["off"], W["length"])
    assert py.matches == want and len({j for o, j, n in want}) == 3
    assert r[0] == dict(matches=[list(m) for m in want], total=len(want), badBlocks=0, firstBadBlock=None, detail="")
    want = rx.expected(plain1, [rb"COURT[a-z]*", rb"[^a-z]s+e"], B - 2, 50000, nocase=True)
    assert r[1]["matches"] == [list(m) for m in want[:7]] and r[1]["total"] == len(want) > 7
    py4 = pkg.Bzip2Index.build(s4, True).search_regex(s4, tiny, off=3)
    want = rx.expected(plain4, tiny, 3)
    assert py4.matches == want and r[2]["matches"] == [list(m) for m in want] and r[2]["total"] == len(want) > 50
    runs = [(0, 7 * 99981), (8 * 99981, plain1.size)]
    assert r[3] == dict(matches=[], total=len(rx.expected(plain1, words[:1], runs=runs)), badBlocks=1, firstBadBlock=7, detail="index does not match the stream at block 7")
    # regexCheck
    st = pkg.regex_check(words + tiny)
    assert rep["check"] == [dict(states=s, maxLen=m) for s, m in st] and rep["checkNocase"] == [dict(states=s, maxLen=m) for s, m in pkg.regex_check(words + tiny, nocase=True)]
    # the refusals: the library's code, and its detail in the message
    ref = rep["refusals"]
    unsupported = dict(anchor="pattern 1, byte 1: anchors", boundary="pattern 1, byte 0: this escaped letter", lazy="pattern 1, byte 2: lazy", states="pattern 1, byte 0: more than 255 states")
    invalid = dict(none="pattern 0, byte 0: 1 to 64 patterns", empty="pattern 1, byte 0: a pattern text outside 1..1024 bytes", matchesEmpty="pattern 1, byte 0: the pattern matches the empty string",
                   paren="pattern 1, byte 0: unbalanced (", bound="pattern 1, byte 1: a repeat bound above 256", long="pattern 1, byte 0: a pattern text outside 1..1024 bytes",
                   check="pattern 1, byte 0: unbalanced [")
    for k, text in unsupported.items():
        assert ref[k]["code"] == rx.E_UNSUPPORTED and ref[k]["error"].startswith("Error:") and text in ref[k]["error"], (k, ref[k])
    for k, text in invalid.items():
        assert ref[k]["code"] == rg.E_INVALID and ref[k]["error"].startswith("Error:") and text in ref[k]["error"], (k, ref[k])
    assert ref["notAnIndex"]["error"].startswith("Error:") and ref["notAnIndex"]["code"] == rg.E_INVALID
    assert ref["fraction"]["error"] == "TypeError:offsets and lengths are integers from 0 to 2^53"
