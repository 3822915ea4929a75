"""The rule of the compress pipeline's pieces (csrc/enc_pieces.h) on the CPU: tests/host/enc_pieces_check.cc (a stand-alone program
with its own main) checks when a call goes in one piece, the default threshold by its constant (level 9: 444 blocks one piece, 445
four), that the pieces of 1..64 blocks tile them in order with none empty, at most four and only the last one short, the piece
sizes of 1..10 and 13 blocks by name, and that nothing overflows at 2^32 - 1 blocks.  It is built with the host compiler under the
address and undefined-behaviour sanitizers and run.  The header also compiles alone, without HIP.  No GPU, nothing loaded into
Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I" + os.path.join(ROOT, "compressjs-flattened_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_enc_pieces_check(tmp_path):
    exe = str(tmp_path / "enc_pieces_check")
    b = subprocess.run(["g++"] + FLAGS + INCLUDES + ["-o", exe, os.path.join(ROOT, "tests", "host", "enc_pieces_check.cc")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("enc_pieces_check ok")


def test_header_compiles_alone_without_hip():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++"] + INCLUDES + ["-"],
                       input='#include "enc_pieces.h"\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
