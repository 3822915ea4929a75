"""Indexed range reads through the JavaScript front (Bzip2.buildIndex / readRange / readRanges) on the GPU: the index bytes are
the Python front's save(), the ranges' bytes are the plaintext's, and a damaged block gives the reference-shaped TypeError."""
import importlib
import json
import os
import re
import shutil
import subprocess

import pytest

import range_cases as rg

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_js_front_matches_the_python_front(tmp_path):
    pkg = importlib.import_module("compressjs-flattened_amd")
    stream, plain, multi, members = rg.f1()
    ix = pkg.Bzip2Index.build(stream)
    e = ix.entries()
    damaged = stream.copy()
    damaged[(e[5][0] + e[5][1]) // 16] ^= 0x04
    src, bad = str(tmp_path / "s.bz2"), str(tmp_path / "bad.bz2")
    stream.tofile(src)
    damaged.tofile(bad)
    ranges = [[5, 10], [99975, 20], [plain.size - 3, 100], [plain.size, 4], [560000, 17], [0, 0], [499900, 100]]
    touch5 = [4, 6]                                         # block 5 is bytes [499905, 599886)
    # the stored CRC of block 5 overwritten in the stream and in the index alike: only the computed one differs
    rows = [list(x) + [0] for x in e]
    real, rows[5][3] = rows[5][3], rows[5][3] ^ 0x00010000
    crc_stream = stream.copy()
    rg.set_bits(crc_stream, rows[5][0] + 48, 32, rows[5][3])
    crc_src = str(tmp_path / "crc.bz2")
    crc_stream.tofile(crc_src)
    job = str(tmp_path / "job.json")
    json.dump({"path": src, "damaged": bad, "multistream": False, "ranges": ranges, "failing": [550000, 5], "crcStream": crc_src,
               "crcIndex": rg.image(rows, stream.size, 0).hex(), "crcRange": [499000, 2000]}, open(job, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_range_check.js"), job], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["indexIsU8"] and bytes.fromhex(rep["index"]) == ix.save()
    want = rg.expected(plain, [tuple(r) for r in ranges])
    assert [r.get("hex") for r in rep["good"]] == [w.hex() for w in want] and all(r["isU8"] for r in rep["good"])
    detail = r"TypeError:Data error: (Bad block CRC \(got [0-9a-f]+ expected %x\)|index does not match the stream at block 5)" % e[5][3]
    for k, r in enumerate(rep["bad"]):
        if k == touch5[0]:                                  # the detail belongs to the lowest failing range
            assert re.fullmatch(detail, r["error"]) and r["code"] == rg.E_DATA, r
        elif k in touch5:
            assert r["error"] == "TypeError:Data error" and r["code"] == rg.E_DATA, r
        else:
            assert r.get("hex") == want[k].hex(), k
    assert rep["one"]["hex"] == want[0].hex()
    assert re.fullmatch(detail, rep["oneBad"]["error"]) and rep["oneBad"]["code"] == rg.E_DATA
    assert rep["notAnIndex"]["error"].startswith("Error:") and rep["notAnIndex"]["code"] == rg.E_INVALID
    assert rep["buildBad"]["error"] == "TypeError:Not bzip data: level out of range"
    assert rep["crc"]["error"] == "TypeError:Data error: Bad block CRC (got %x expected %x)" % (real, rows[5][3]) and rep["crc"]["code"] == rg.E_DATA
    for k in ("fraction", "fractionLen"):                   # (no silent truncation to 10 or 0)
        assert rep[k]["error"] == "TypeError:offsets and lengths are integers from 0 to 2^53", rep[k]
