"""The narrow phase-1 record of the packed cyclic round 1 (csrc/bwt_rules.h) on the CPU: tests/host/bwt_pk1_check.cc (a stand-alone
program with its own main) round-trips the 32-bit record byte 2 | position for every position up to 2^20 - 3 with every byte 2,
checks that pk_pos reads the same position from the 8-byte record, its narrowed form and the phase-2 record, that narrowing
keeps byte 2 whatever the rest of the key holds, that the records order as (byte 2, position), and that the class key and the
phase-2 fields formed from eight text bytes are the ones the 8-byte record carried.  Built with the host compiler under the address
and undefined-behaviour sanitizers.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narrow_record_by_property(tmp_path):
    exe = str(tmp_path / "bwt_pk1_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "host", "bwt_pk1_check.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("bwt_pk1_check ok")
