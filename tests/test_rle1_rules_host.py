"""The host-visible arithmetic of stage 0 (csrc/rle1_rules.h, csrc/crc32_bz.h) on the CPU: tests/host/rle1_rules_check.cc (a stand-alone
program with its own main) checks by property, against a byte-serial model of the block reader's run handling, the chunk rule, the
bytes a freshly chunked run emits and where each of its bytes goes, and the input length at which one run fills a block (every
capacity 1..5000 and the nine real ones); the layout of the multi-GPU tile-table share (sections in order, disjoint, aligned for
their 16-byte reads); and, against a bit-by-bit CRC, the CRC tables, the GF(2) multiply and powers, the check value, and
partial-then-final over the shared address-window function on a few thousand random ranges, each touching at most crc_segs_for
windows.  It is built with the host compiler under the address and undefined-behaviour sanitizers.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rle1_rules_by_property(tmp_path):
    exe = str(tmp_path / "rle1_rules_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "host", "rle1_rules_check.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("rle1_rules_check ok")
