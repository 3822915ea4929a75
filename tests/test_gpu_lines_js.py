"""The line table through the JavaScript front (Bzip2.buildLineIndex, lineStarts, lineNumbers, readLines) on the GPU, on F1 and
LN2: every value is numpy's over the decoded text, passed in and compared here; one case reads a stream with a damaged block."""
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


def _case(path, multi, plain, bounds, damaged=None):
    nl, total, N = lc.newlines(plain), int(plain.size), int(lc.newlines(plain).size)
    rng = np.random.RandomState(3)
    lines = [0, 1, 2, N - 1, N, N + 1, 2 ** 53] + rng.randint(0, N + 2, 300).tolist()
    offsets = [0, total - 1, total, total + 7, 2 ** 53] + [int(b) + d for b in bounds[1:-1][:20] for d in (-1, 0, 1)] + rng.randint(0, total, 300).tolist()
    mid = lc.number(nl, total, int(bounds[len(bounds) // 2]))
    spans = [[0, 1], [N - 1, 1], [N, 1], [max(mid - 1, 0), 3], [N - 1, 10], [N + 5, 2], [0, N + 1]]
    return dict(path=path, multistream=bool(multi), lines=[int(x) for x in lines], offsets=[int(x) for x in offsets], spans=spans, damaged=damaged)


def _block_of(bounds, o):
    return int(np.searchsorted(bounds, o, "right")) - 1


def test_js_lines_match_numpy(tmp_path):
    oracle = support.Oracle()
    f1, plain1, _, _ = rg.f1()
    s2, plain2, _ = lc.ln2(oracle)
    src1, src2, bad1 = str(tmp_path / "f1.bz2"), str(tmp_path / "ln2.bz2"), str(tmp_path / "bad.bz2")
    f1.tofile(src1)
    s2.tofile(src2)
    rc, tab1 = oracle.bzip2_table(f1, 0)
    assert rc == 0
    damaged = f1.copy()
    rg.set_bits(damaged, tab1[7][0], 48, 0x314159265358)      # the magic of block 7
    damaged.tofile(bad1)
    b1, b2 = lc.oracle_bounds(oracle, f1, 0), lc.oracle_bounds(oracle, s2, 1)
    cases = [_case(src1, 0, plain1, b1, damaged=bad1), _case(src1, 0, plain1, b1), _case(src2, 1, plain2, b2)]
    job = str(tmp_path / "job.json")
    json.dump({"cases": cases}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_lines_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    text7 = "index does not match the stream at block 7"
    for c, r, plain, bounds in zip(cases, rep["cases"], (plain1, plain1, plain2), (b1, b1, b2)):
        nl, total, N = lc.newlines(plain), int(plain.size), int(lc.newlines(plain).size)
        counts = lc.block_counts(plain, bounds)
        assert bytes.fromhex(r["table"])[40:] == np.asarray(counts, "<u4").tobytes() and bytes.fromhex(r["table"])[:8] == b"CJSBZLN1"
        bad = {7} if c["damaged"] else set()
        starts = set(int(x) for x in bounds)
        kb = [_block_of(bounds, int(nl[k - 1])) if 1 <= k <= N else -1 for k in c["lines"]]
        ob = [_block_of(bounds, o) if o < total and o not in starts else -1 for o in c["offsets"]]
        assert r["starts"]["values"] == [0 if b in bad else lc.start(nl, total, k) for k, b in zip(c["lines"], kb)]
        assert r["starts"]["status"] == [rg.E_DATA if b in bad else 0 for b in kb]
        assert r["numbers"]["values"] == [0 if b in bad else lc.number(nl, total, o) for o, b in zip(c["offsets"], ob)]
        assert r["numbers"]["status"] == [rg.E_DATA if b in bad else 0 for b in ob]
        assert r["starts"]["detail"] == r["numbers"]["detail"] == (text7 if bad else "")
        if bad:
            assert any(b in bad for b in kb) and any(b in bad for b in ob)
        for (a, n), got in zip(c["spans"], r["spans"]):
            lo, hi = lc.start(nl, total, a), lc.start(nl, total, a + n)
            if bad and any(_block_of(bounds, o) in bad for o in (lo, hi - 1) if lo < hi) or (bad and lo <= bounds[7] and hi >= bounds[8]):
                assert got == dict(error="TypeError:Data error: " + text7, code=rg.E_DATA), (a, n, got)
            else:
                assert got == plain[lo:hi].tobytes().hex(), (a, n)
    ref = rep["refusals"]
    for k in ("fraction", "negative"):
        assert ref[k]["error"] == "TypeError:line numbers and offsets are integers from 0 to 2^53", (k, ref[k])
    for k in ("notATable", "foreign"):
        assert ref[k]["error"].startswith("Error:") and ref[k]["code"] == rg.E_INVALID, (k, ref[k])
    assert ref["damagedBuild"] == dict(error="TypeError:Data error: " + text7, code=rg.E_DATA)
