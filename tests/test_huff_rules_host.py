"""The host-visible rules of the entropy stage (csrc/huff_rules.h) on the CPU: tests/host/huff_rules_check.cc (a stand-alone program
with its own main, linked with the oracle) checks the code-length allocator -- pass 1 and the one template of passes 2 and 3, with
serial callables -- against the oracle's allocator on 63,000 sorted frequency vectors of five families at the limits 20 and 32
(at least a tenth of them reach the limit, at least 1,000 take the relocation branch), the rank-sort key against the oracle's
lengths, a few hundred small blocks written item by item (header, selectors, delta-coded tables, canonical codes) against the
oracle's block bits bit for bit and against block_bits, the geometry, the frame and the workspace layout against the literal
formulas they replaced, and the bit splitter against a bit-by-bit writer.  It is built with the host compiler under the address
and undefined-behaviour sanitizers.  No GPU, no HIP, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_huff_rules_against_the_oracle(tmp_path):
    obj, exe = str(tmp_path / "cjs_oracle.o"), str(tmp_path / "huff_rules_check")
    b = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror"] + SANITIZE + ["-c", "-o", obj, os.path.join(ROOT, "oracle", "cjs_oracle.c")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + SANITIZE + INCLUDES +
                       ["-o", exe, os.path.join(ROOT, "tests", "host", "huff_rules_check.cc"), obj], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("huff_rules_check ok")


def test_header_compiles_alone_without_hip():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"] + INCLUDES[:2] + ["-"],
                       input='#include "huff_rules.h"\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
