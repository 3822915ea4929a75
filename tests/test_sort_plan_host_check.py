"""The rule of the line sort (csrc/sort_plan.h) on the CPU: tests/host/sort_plan_check.cc (a stand-alone program with its own main)
checks sl_word against a byte-wise restatement at every len - d in -2..9 with 0x00 / 0xFF content, the rounds of sl_sort_host
against std::stable_sort with memcmp on 400 random texts under all flags and short caps, the tail rule and the argument errors.  It
is built with the host compiler under the address and undefined-behaviour sanitizers and run.  The header also compiles alone,
without HIP.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_sort_plan_check(tmp_path):
    exe = str(tmp_path / "sort_plan_check")
    b = subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(ROOT, "tests", "host", "sort_plan_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("sort_plan_check ok")


def test_header_compiles_alone_without_hip():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"] + INCLUDES + ["-"],
                       input='#include "sort_plan.h"\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
