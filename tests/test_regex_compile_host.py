"""The pattern compiler of the regex search (csrc/rx_compile.h) on the CPU: tests/host/rx_compile_check.cc (a stand-alone program with
its own main) compares the compiled tables, walked as the kernels walk them, with a matcher of its own over a few thousand random
patterns from a small grammar and random texts over a 4-letter alphabet plus the newline, and checks on patterns built for it every
refusal of the contract (code, and a detail that names pattern and byte), max_len and the state counts, the class map, the clamp at
256 bytes and that nothing in a blob points outside it.  It is built with the host compiler under the address and
undefined-behaviour sanitizers.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_regex_compiler_against_a_matcher(tmp_path):
    exe = str(tmp_path / "rx_compile_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "host", "rx_compile_check.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("rx_compile_check ok")
