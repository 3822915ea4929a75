"""The arithmetic of the column cut (csrc/cut_plan.h) on the CPU: tests/host/cut_plan_check.cc (a stand-alone program with its own
main) checks the list parser with every refusal, the normal form, membership against a naive set, the summary monoid's associativity
on random three-way splits, the pieces of random texts cut with the carried state against cut_text of the whole, the saturating
counter, and cut_text against a second implementation.  It is built with the host compiler under the address and
undefined-behaviour sanitizers and run.  The header also compiles alone, without HIP.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_cut_plan_check(tmp_path):
    exe = str(tmp_path / "cut_plan_check")
    b = subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(ROOT, "tests", "host", "cut_plan_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("cut_plan_check ok")


def test_header_compiles_alone_without_hip():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"] + INCLUDES + ["-"],
                       input='#include "cut_plan.h"\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
