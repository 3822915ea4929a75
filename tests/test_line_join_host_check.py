"""The join of the line keys (csrc/line_join.h) on the CPU: tests/host/line_join_check.cc (a stand-alone program with its own main)
runs LkJoin over 400 random texts cut into random blocks, with random windows, caps and bad blocks, to both destinations and under
both tail rules, against lk_text_keys of the whole text, and checks text_keys_work_bytes against the layout of the pieces and tiles
a text really has.  It is built with the host compiler under the address and undefined-behaviour sanitizers and run.  The header
also compiles alone, without HIP.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_line_join_check(tmp_path):
    exe = str(tmp_path / "line_join_check")
    b = subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(ROOT, "tests", "host", "line_join_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("line_join_check ok")


def test_header_compiles_alone_without_hip():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"] + INCLUDES + ["-"],
                       input='#include "line_join.h"\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
