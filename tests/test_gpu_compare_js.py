"""Compare through the JavaScript front (Bzip2.compare, Bzip2.compareStreams) on the GPU, on F1: the lists are numpy's over the
decoded text -- equal, flips, a window, a cap, a shorter other side, a damaged block, and a second stream whose blocks fall
differently."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import range_cases as rg
import support

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _objects(want):
    return [dict(offset=o, a=a, b=b) for o, a, b in want]


def test_js_compare_matches_numpy(tmp_path):
    oracle = support.Oracle()
    f1, plain, _, _ = rg.f1()
    total = plain.size
    rc, tab = oracle.bzip2_table(f1, 0)
    assert rc == 0
    bounds = np.concatenate([[0], np.cumsum([t[1] for t in tab])]).astype(np.int64)
    B = int(bounds[3])
    other = cc.flipped(plain, cc.seam_flips(bounds) + cc.random_flips(total, 120, 61), seed=13)
    rc, s9 = oracle.bzip2_compress(other, 9)
    assert rc == 0
    damaged = f1.copy()
    rg.set_bits(damaged, tab[7][0], 48, 0x314159265358)      # the magic of block 7
    src, bad, same, flip, twin = (str(tmp_path / n) for n in ("f1.bz2", "bad.bz2", "same.bin", "flip.bin", "twin.bz2"))
    f1.tofile(src), damaged.tofile(bad), plain.tofile(same), other.tofile(flip), np.asarray(s9, dtype=np.uint8).tofile(twin)
    cases = [
        dict(path=src, multistream=False, other=same, opts={}),
        dict(path=src, multistream=False, other=flip, opts={"limit": None}),
        dict(path=src, multistream=False, other=flip, opts={"offset": B - 5, "length": 40000}),                       # the default limit
        dict(path=src, multistream=False, other=flip, slice=[B - 100, B + 20000], opts={"otherOffset": B - 100, "limit": 3}),      # a shorter other side, a cap
        dict(path=src, multistream=False, other=flip, opts={"limit": 0}, damaged=bad),
        dict(path=src, multistream=False, otherStream=twin, opts={"limit": None}),
        dict(path=src, multistream=False, otherStream=src, opts={"offset": 5, "length": 500000}),
        dict(path=src, multistream=False, other=same, slice=[0, total - 9], opts={}),
    ]
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_compare_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    r = rep["cases"]
    none = dict(badBlocks=0, firstBadBlock=None, badBlocksB=0, firstBadBlockB=None, detail="")
    assert r[0] == dict(equal=True, diffs=[], total=0, firstDiff=None, compared=total, lenA=total, lenB=total, **none)
    want, compared = cc.expected(plain, other)
    assert len(want) > 150
    assert r[1] == dict(equal=False, diffs=_objects(want), total=len(want), firstDiff=0, compared=total, lenA=total, lenB=total, **none)
    want, compared = cc.expected(plain, other, off=B - 5, ln=40000)
    assert r[2]["diffs"] == _objects(want[:64]) and (r[2]["total"], r[2]["firstDiff"], r[2]["compared"]) == (len(want), want[0][0], 40000) and not r[2]["equal"]
    want, compared = cc.expected(plain, other[B - 100:B + 20000], B - 100)
    assert r[3]["diffs"] == _objects(want[:3]) and (r[3]["total"], r[3]["compared"], r[3]["lenB"]) == (len(want), 20100, B + 20000) and len(want) > 3
    want, compared = cc.expected(plain, other, runs=[(0, int(bounds[7])), (int(bounds[8]), total)])
    assert r[4] == dict(equal=False, diffs=[], total=len(want), firstDiff=0, compared=compared, lenA=total, lenB=total, badBlocks=1, firstBadBlock=7,
                        badBlocksB=0, firstBadBlockB=None, detail="index does not match the stream at block 7")
    want, compared = cc.expected(plain, other)
    assert r[5] == dict(equal=False, diffs=_objects(want), total=len(want), firstDiff=0, compared=total, lenA=total, lenB=total, **none)
    assert r[6] == dict(equal=False, diffs=[], total=0, firstDiff=None, compared=500000, lenA=total, lenB=total, **none)      # a window is not the whole
    assert r[7] == dict(equal=False, diffs=[], total=0, firstDiff=None, compared=total - 9, lenA=total, lenB=total - 9, **none)
    ref = rep["refusals"]
    for k in ("fraction", "negative"):
        assert ref[k]["error"] == "TypeError:offsets and lengths are integers from 0 to 2^53", (k, ref[k])
    for k in ("notAnIndex", "otherIndex", "wrongStream"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
