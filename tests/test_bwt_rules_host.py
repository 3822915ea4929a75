"""The rules of the suffix sort (csrc/bwt_rules.h) on the CPU: tests/host/bwt_rules_check.cc (a stand-alone program with its own main)
walks every tile-sorter window of 3,000 random group-size sequences -- sizes from {2, 3, 63, 64, 65, 1023, 1024, 1025, 3071, 3072, 3073,
5000} and random ones, starts on and around multiples of the nominal range, array ends inside a window's slack -- with the header's
functions only and checks against a serial model: one owner window per slot of a group of <= 1024 members, holding the whole group;
no owner for larger groups; one window that fetches each slot's rank; prev_end of every window; the large-group flag (all three
forms agree, it is raised for every group of more than 1023 slots at every alignment and never without a group of more than 512);
every record layout round-trips with no field overlapping another; round-1 key arithmetic for every block count 1..70,000 in both
forms and geometries; bits_for and the round stepping.  It is built with the host compiler under the address and
undefined-behaviour sanitizers.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bwt_rules_by_property(tmp_path):
    exe = str(tmp_path / "bwt_rules_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "host", "bwt_rules_check.cc")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("bwt_rules_check ok")
