"""The column cut through the JavaScript front (Bzip2.cutLines) on the GPU, on CT1 and CT2: every call's bytes are the Python
front's (whose bytes test_gpu_cut.py holds against the restatement) for four selections and a window; one case reads a stream with a
damaged block; then the refusals' messages and errorCode."""
import importlib
import json
import os
import shutil
import subprocess

import pytest

import cut_cases as ct
import lines_cases as lc
import range_cases as rg
import support

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [dict(fields="2"), dict(fields="1,3-5"), dict(fields=[[3, None], 1]), dict(bytes="2,4,70-90"), dict(fields="2-3", first=9, count=200),
         dict(fields="1", delimiter=","), dict(fields="2", delimiter=0)]


def _py(o):
    kw = dict(o)
    for k in ("fields", "bytes"):
        if isinstance(kw.get(k), list):
            kw[k] = [tuple(x) if isinstance(x, list) else x for x in kw[k]]
    return kw


def test_js_cut_matches_the_python_front(tmp_path):
    pkg = importlib.import_module("compressjs-flattened_amd")
    oracle = support.Oracle()
    s1, plain1, _ = ct.ct1(oracle)
    s2, plain2, _ = ct.ct2(oracle)
    rc, tab1 = oracle.bzip2_table(s1, 0)
    assert rc == 0
    damaged = s1.copy()
    rg.set_bits(damaged, tab1[1][0], 48, 0x314159265358)      # the magic of block 1
    paths = {k: str(tmp_path / (k + ".bz2")) for k in ("ct1", "ct2", "bad")}
    for k, s in (("ct1", s1), ("ct2", s2), ("bad", damaged)):
        s.tofile(paths[k])
    last = int(lc.newlines(plain1).size) - 50
    cases = [dict(path=paths["ct1"], multistream=False, damaged=None, calls=CALLS),
             dict(path=paths["ct2"], multistream=True, damaged=None, calls=CALLS),
             dict(path=paths["ct1"], multistream=False, damaged=paths["bad"], calls=[dict(fields="2"), dict(fields="2", first=0, count=100), dict(fields="2", first=last)])]
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_cut_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])

    made = {}
    for k, (s, multi) in {"ct1": (s1, False), "ct2": (s2, True)}.items():
        ix = pkg.Bzip2Index.build(s, multi)
        made[k] = (s, ix, pkg.Bzip2Lines.build(s, ix))
    for c, r, name in zip(cases[:2], rep["cases"], ("ct1", "ct2")):
        s, ix, ln = made[name]
        for o, got in zip(c["calls"], r):
            want = ix.cut_lines(s, ln, **_py(o))
            assert got == dict(isBuffer=True, hex=want.hex()), (name, o, got.get("error"))
        assert len(r[0]["hex"]) > 1000
    s, ix, ln = made["ct1"]
    whole, front, behind = rep["cases"][2]
    text1 = "index does not match the stream at block 1"
    assert whole == dict(error="TypeError:Data error: " + text1, code=rg.E_DATA), whole
    assert front["hex"] == ix.cut_lines(s, ln, fields="2", first=0, count=100).hex() and behind["hex"] == ix.cut_lines(s, ln, fields="2", first=last).hex()

    ref = rep["refusals"]
    assert ref["neither"]["error"] == ref["both"]["error"] == "TypeError:exactly one of fields and bytes must be given"
    assert ref["wideDelimiter"]["error"] == "TypeError:the delimiter is one byte"
    assert ref["fraction"]["error"] == "TypeError:first and count are integers from 0 to 2^53"
    for k in ("zero", "notAList", "backwards", "newline"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
    assert ref["foreign"]["error"].startswith("Error:") and ref["foreign"]["code"] == rg.E_INVALID
