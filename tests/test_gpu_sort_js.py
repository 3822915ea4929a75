"""The line sort through the JavaScript front (Bzip2.sortLines) on the GPU, on TL1: every entry, counter and text is the Python
front's (which test_gpu_sort.py holds against sorted() over the real lines), whole lines and the sort of a cut; a stream with a
damaged block, and the refusals."""
import importlib
import json
import os
import shutil
import subprocess

import pytest

import range_cases as rg
import support
import tally_cases as tc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_js_sort_matches_the_python_front(tmp_path):
    pkg = importlib.import_module("compressjs-flattened_amd")
    oracle = support.Oracle()
    stream, plain, _ = tc.tl1(oracle)
    N = plain.tobytes().count(b"\n")
    rc, tab = oracle.bzip2_table(stream, 0)
    assert rc == 0
    damaged = stream.copy()
    rg.set_bits(damaged, tab[1][0], 48, 0x314159265358)      # the magic of block 1
    paths = {k: str(tmp_path / (k + ".bz2")) for k in ("tl1", "bad")}
    stream.tofile(paths["tl1"])
    damaged.tofile(paths["bad"])
    calls = [{"first": 15, "count": 3000}, {"limit": 16, "first": 15, "count": 3000, "text": True}, {"unique": True, "first": 20, "count": 5000},
             {"reverse": True, "unique": True, "limit": 7, "first": 20, "count": 5000}, {"first": N, "limit": 2}, {"first": N + 1, "text": True}, {"limit": 0, "count": 50},
             {"first": 100, "count": 2 ** 53, "limit": 3, "reverse": True}, {"fields": "2", "limit": 8, "first": 15, "count": 3000, "text": True},
             {"bytes": [[1, 8]], "delimiter": "\t", "unique": True, "first": 15, "count": 4000}]
    job = str(tmp_path / "job.json")
    json.dump({"path": paths["tl1"], "multistream": False, "calls": calls, "damaged": paths["bad"]}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_sort_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])

    ix = pkg.Bzip2Index.build(stream)
    ln = pkg.Bzip2Lines.build(stream, ix)
    for o, got in zip(calls, rep["calls"]):
        assert "error" not in got, got
        kw = {{"text": "want_text"}.get(k, k): v for k, v in o.items()}
        res = ix.sort_lines(stream, ln, **kw)
        assert got["lines"] == res.lines.tolist() and got["counts"] == res.counts.tolist(), o
        assert (got["nLines"], got["nOut"], got["nDistinct"], got["textBytes"], got["rounds"]) == (res.n_lines, res.n_out, res.n_distinct, res.text_bytes, res.rounds)
        assert got["text"] == (res.text.hex() if o.get("text") else None)
    c = rep["calls"]
    assert c[0]["nLines"] == 3000 == len(c[0]["lines"]) and len(c[1]["lines"]) == 16 and c[1]["lines"] == c[0]["lines"][:16] and c[5]["nLines"] == 0 and c[5]["text"] == ""
    assert c[6]["lines"] == [] and c[6]["nOut"] == 50 and sum(c[2]["counts"]) == 5000 and c[8]["nDistinct"] < c[0]["nDistinct"]
    assert rep["damaged"] == dict(error="TypeError:Data error: index does not match the stream at block 1", code=rg.E_DATA)
    ref = rep["refusals"]
    assert ref["both"]["error"] == "TypeError:at most one of fields and bytes may be given"
    for k in ("fraction", "negative"):
        assert ref[k]["error"] == "TypeError:first, count and limit are integers from 0 to 2^53", (k, ref[k])
    for k in ("list", "foreign"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
