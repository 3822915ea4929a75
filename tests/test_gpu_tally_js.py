"""The line frequency table through the JavaScript front (Bzip2.tallyLines) on the GPU, on TL1: every group and every counter is
the Python front's (which test_gpu_tally.py holds against collections.Counter over the real lines), whole lines and the tally of a
cut; a stream with a damaged block in both, and the refusals."""
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import range_cases as rg
import support
import tally_cases as tc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_js_tally_matches_the_python_front(tmp_path):
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
    calls = [{}, {"limit": 16}, {"order": "first", "minCount": 2}, {"order": "first", "maxCount": 1, "seed": 77}, {"first": 5, "count": 1000, "limit": 3},
             {"first": N, "limit": 2}, {"first": N + 1}, {"limit": 0}, {"minCount": 2, "maxCount": 3, "order": "count", "first": 100, "count": 2 ** 53},
             {"fields": "2", "limit": 8}, {"fields": [1, 3], "order": "first", "minCount": 2}, {"bytes": [[1, 8]], "delimiter": "\t", "limit": 5, "first": 7, "count": 4000}]
    job = str(tmp_path / "job.json")
    json.dump({"path": paths["tl1"], "multistream": False, "calls": calls, "damaged": paths["bad"]}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_tally_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])

    ix = pkg.Bzip2Index.build(stream)
    ln = pkg.Bzip2Lines.build(stream, ix)
    names = {"minCount": "min_count", "maxCount": "max_count"}
    ref = rep["refusals"]

    def same(got, res):
        assert "error" not in got, got
        assert got["groups"] == res.groups.tobytes().hex()
        assert (got["nLines"], got["nDistinct"], got["nGroups"], got["nBadLines"], got["maxCount"]) == (res.n_lines, res.n_distinct, res.n_groups, res.n_bad_lines, res.max_count)
        assert got["badBlocks"] == res.bad_blocks and got["firstBadBlock"] == res.first_bad_block and got["detail"] == res.detail

    for o, got in zip(calls, rep["calls"]):
        same(got, ix.tally_lines(stream, ln, **{names.get(k, k): v for k, v in o.items()}))
    assert rep["calls"][0]["nLines"] == N + 1 and len(rep["calls"][1]["groups"]) == 16 * 64 and rep["calls"][6]["nLines"] == 0 and rep["calls"][7]["groups"] == ""
    assert rep["calls"][9]["nDistinct"] < rep["calls"][0]["nDistinct"] and len(rep["calls"][9]["groups"]) == 8 * 64
    bad = ix.tally_lines(damaged, ln, limit=5)
    same(rep["damaged"], bad)
    assert rep["damagedCut"] == dict(error="TypeError:Data error: index does not match the stream at block 1", code=rg.E_DATA)
    assert ref["both"]["error"] == "TypeError:at most one of fields and bytes may be given"
    assert bad.bad_blocks == 1 and bad.first_bad_block == 1 and bad.n_bad_lines > 0 and bad.detail == "index does not match the stream at block 1"
    for k in ("fraction", "negative"):
        assert ref[k]["error"] == "TypeError:first, count, seed, minCount, maxCount and limit are integers from 0 to 2^53", (k, ref[k])
    assert ref["order"]["error"] == "TypeError:order is 'count' or 'first'"
    for k in ("filter", "foreign"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
