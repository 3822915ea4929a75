"""The host arithmetic of the indexed consumers (csrc/scan_plan.h) on the CPU: tests/host/scan_plan_check.cc (a stand-alone program
with its own main) checks by property, against brute-force models on a few thousand random cases each, the window clamp and the
blocks under a window, the good blocks of a batch as runs (exactly the window's bytes of the good blocks, in order, merged only
where adjacent in offset and address), the intersection of two sides' runs (exactly the common bytes, both addresses, dense tile
numbers), the search's segments and carry over whole calls cut into random batches (every start position of a good run tested
exactly once, with enough bytes behind it; the carry bounded and continuing its run) and the routing of both line questions.  It is
built with the host compiler under the address and undefined-behaviour sanitizers.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_plans_by_property(tmp_path):
    exe = str(tmp_path / "scan_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "host", "scan_plan_check.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("scan_plan_check ok")
