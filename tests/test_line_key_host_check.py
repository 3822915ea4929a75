"""The arithmetic of the line keys and the line diff (csrc/line_key.h, csrc/line_diff.h) on the CPU: tests/host/line_key_check.cc (a
stand-alone program with its own main) checks the mulmod, the power and the join against naive 128-bit arithmetic, the join's
associativity on random splits, the keys of a text, and the diff against the quadratic DP on random pairs and on the recursion's
ends.  It is built with the host compiler under the address and undefined-behaviour sanitizers and run.  Both headers also compile
alone, without HIP.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_line_key_check(tmp_path):
    exe = str(tmp_path / "line_key_check")
    b = subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(ROOT, "tests", "host", "line_key_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("line_key_check ok")


@pytest.mark.parametrize("header", ("line_key.h", "line_diff.h"))
def test_header_compiles_alone_without_hip(header):
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"] + INCLUDES + ["-"],
                       input='#include "%s"\n' % header, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
