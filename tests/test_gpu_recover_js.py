"""Bzip2 recovery through the JavaScript front and the command line (Bzip2.recoverFile, cli.js --recover / --repair) on the GPU:
the same bytes and the same rows as the C ABI gives for the same damaged input."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import recover_cases as rc_
import support

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(support.PKG, "js")


@pytest.fixture(scope="module")
def L():
    return rc_.bind(os.path.join(support.PKG, "libcjs_hip.so"))


def _inputs(oracle):
    return {"flipped-bit": rc_.damage_a(oracle), "forty-every-third": rc_.forty_damaged(oracle, "every-third")[0]}


def test_js_front_matches_the_c_abi(L, oracle, tmp_path):
    jobs = []
    for name, buf in _inputs(oracle).items():
        path = str(tmp_path / (name + ".bz2"))
        buf.tofile(path)
        jobs.append({"name": name, "path": path})
    jf = str(tmp_path / "jobs.json")
    json.dump(jobs, open(jf, "w"))
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js_recover_check.js"), jf], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["shadowed"] == 1 and len(rep["results"]) == 2
    for r in rep["results"]:
        buf = _inputs(oracle)[r["name"]]
        for as_stream in (0, 1):
            rc, want, found = rc_.recover_host(L, buf, as_stream)
            form = r["forms"][as_stream]
            assert rc == 0 and form["isU8"] and form["len"] == len(want) and form["sha256"] == hashlib.sha256(want).hexdigest(), r["name"]
            assert form["rows"] == [[f[0], f[3], f[4]] for f in found] and any(f[4] == 0 for f in found) and any(f[4] < 0 for f in found)
        assert r["sinkReturned"] is True and r["sinkLen"] == r["forms"][0]["len"]
        assert r["shortOut"] == "TypeError:outputsize does not match decoded input"


@pytest.mark.parametrize("flag, as_stream", [("--recover", 0), ("--repair", 1)])
def test_cli_writes_the_recovered_bytes(L, oracle, tmp_path, flag, as_stream):
    bad = rc_.damage_a(oracle)
    src, dst = str(tmp_path / "bad.bz2"), str(tmp_path / "out.bin")
    bad.tofile(src)
    rc, want, found = rc_.recover_host(L, bad, as_stream)
    assert rc == 0
    out = subprocess.run(["node", os.path.join(JS, "cli.js"), flag, "-t", "bzip2", src, dst], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert open(dst, "rb").read() == want
    assert out.stderr.strip() == "recovered 2 of 3 blocks (%d bytes)" % len(want) and out.stdout == ""
