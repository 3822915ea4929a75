"""The line keys and the line diff through the JavaScript front (Bzip2.lineKeys, Bzip2.diffLines) on the GPU, on F1 and LN2: every
record and every hunk is the Python front's (whose records test_gpu_linekeys.py holds against the restated key); one case reads a
stream with a damaged block, one passes a table that is not the index's."""
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import lines_cases as lc
import range_cases as rg
import support

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 77


def test_js_line_keys_match_the_python_front(tmp_path):
    pkg = importlib.import_module("compressjs-flattened_amd")
    oracle = support.Oracle()
    f1, plain1, _, _ = rg.f1()
    s2, plain2, _ = lc.ln2(oracle)
    lines1 = plain1.tobytes().split(b"\n")
    edited = b"\n".join(lines1[:5] + [b"a new line"] + lines1[5:40000] + lines1[40003:90000] + [b"changed"] + lines1[90001:])
    rc, sb = oracle.bzip2_compress(np.frombuffer(edited, dtype=np.uint8), 9)
    assert rc == 0
    sb = np.asarray(sb, dtype=np.uint8)
    rc, tab1 = oracle.bzip2_table(f1, 0)
    assert rc == 0
    damaged = f1.copy()
    rg.set_bits(damaged, tab1[7][0], 48, 0x314159265358)      # the magic of block 7
    paths = {k: str(tmp_path / (k + ".bz2")) for k in ("f1", "ln2", "b", "bad")}
    for k, s in (("f1", f1), ("ln2", s2), ("b", sb), ("bad", damaged)):
        s.tofile(paths[k])
    N1, N2 = int(lc.newlines(plain1).size), int(lc.newlines(plain2).size)
    w1 = [[0, None], [0, 0], [N1, 1], [N1 + 1, 5], [1000, 20000], [N1 - 3, 2 ** 53]]
    w2 = [[0, None], [3, 7], [N2, None], [0, N2]]
    cases = [dict(path=paths["f1"], multistream=False, windows=w1, seed=SEED, other=paths["b"], damaged=None),
             dict(path=paths["ln2"], multistream=True, windows=w2, seed=0, other=None, damaged=None),
             dict(path=paths["f1"], multistream=False, windows=[[0, None], [0, 10]], seed=SEED, other=paths["b"], damaged=paths["bad"])]
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_linekeys_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])

    streams = {"f1": (f1, False), "ln2": (s2, True), "b": (sb, False)}
    made = {}
    for k, (s, multi) in streams.items():
        ix = pkg.Bzip2Index.build(s, multi)
        made[k] = (s, ix, pkg.Bzip2Lines.build(s, ix))
    text7 = "index does not match the stream at block 7"
    for c, r, name in zip(cases, rep["cases"], ("f1", "ln2", "f1")):
        s, ix, ln = made[name]
        target = damaged if c["damaged"] else s
        for (first, count), got in zip(c["windows"], r["windows"]):
            keys, info = ix.line_keys(target, ln, first=first, count=count, seed=c["seed"])
            assert got["keys"] == keys.tobytes().hex() and got["lines"] == info.n_lines == keys.size, (name, first, count)
            assert got["badBlocks"] == info.bad_blocks and got["firstBadBlock"] == info.first_bad_block and got["detail"] == info.detail
        if c["damaged"]:
            assert r["windows"][0]["badBlocks"] == 1 and r["windows"][0]["firstBadBlock"] == 7 and r["windows"][0]["detail"] == text7
            assert "ff" * 16 in r["windows"][0]["keys"] and r["windows"][1]["badBlocks"] == 0
            assert r["diff"] == dict(error="TypeError:Data error: " + text7, code=rg.E_DATA)
        elif c["other"]:
            sb_, ixb, lnb = made["b"]
            res = ix.diff_stream(s, ln, sb_, ixb, lnb, seed=c["seed"])
            assert [(h["aFirst"], h["aCount"], h["bFirst"], h["bCount"]) for h in r["diff"]["hunks"]] == res.hunks == [(5, 0, 5, 1), (40000, 3, 40001, 0), (90000, 1, 89998, 1)]
            assert (r["diff"]["edits"], r["diff"]["common"], r["diff"]["minimal"]) == (res.edits, res.common, True) and res.edits == 6
            capped = ix.diff_stream(s, ln, sb_, ixb, lnb, max_edits=2, seed=c["seed"])
            assert r["diffCapped"]["minimal"] is False and not capped.minimal and len(r["diffCapped"]["hunks"]) == 1
            assert [(h["aFirst"], h["aCount"], h["bFirst"], h["bCount"]) for h in r["diffCapped"]["hunks"]] == capped.hunks
            assert r["same"] == dict(hunks=[], edits=0, common=len(lines1) - 3, minimal=True)
    ref = rep["refusals"]
    for k in ("fraction", "negative"):
        assert ref[k]["error"] == "TypeError:first, count and seed are integers from 0 to 2^53", (k, ref[k])
    for k in ("notATable", "foreign"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
