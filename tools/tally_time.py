#!/usr/bin/env python3
"""The line frequency table of a .bz2 stream against what it rides on and what a user does without it, every result checked
against collections.Counter over the real lines before anything is timed.  One JSON line per group.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1), its index and its line table.
  device   tally_lines_device of the whole stream, the 10 most frequent: whole lines, fields 1 and bytes 1-16 (delimiter b" ")
           against   line_keys_device (the same decode and the same keys, the records brought down) and cut_lines_device of the
           same selections (the first step of the tally of a cut): the yardsticks
  host     Bzip2Index.tally_lines (the stream in host memory)   against   cjs_bzip2_decompress plus collections.Counter in Python
           (one run)
  keys     tally_keys on the stream's keys (host memory: upload, grouping, 10 groups back)   against   numpy.unique on the host
The ways alternate in one process after a warm-up of each: median and spread (max - min) of --reps runs.

--one-call makes one tally_lines_device call of the whole stream and nothing else: the program for a kernel trace of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -d tool_out/tally_trace -- python tools/tally_time.py [MB] --one-call
whose stats give the share of the radix passes and of the tl_* kernels in the call.

usage: python tools/tally_time.py [MB] [--reps 5]
"""
import argparse
import collections
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TOP = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", action="store_true", help="one tally_lines_device call of the whole stream and nothing else")
    a = ap.parse_args()
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(a.mb * 1000000, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    ix = pkg.Bzip2Index.build(stream)
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    ptr, n = d_in.data_ptr(), stream.size
    table = pkg.lines_build_device(ptr, n, ix)
    on_device = lambda **cut: pkg.tally_lines_device(ptr, n, ix, table, limit=TOP, **cut)
    CUTS = {"fields 1": dict(fields="1", delimiter=b" "), "bytes 1-16": dict(bytes="1-16", delimiter=b" ")}
    d_out = torch.empty(data.size + 1, dtype=torch.uint8, device="cuda")
    cut_device = lambda **cut: pkg.cut_lines_device(ptr, n, ix, table, d_out_ptr=d_out.data_ptr(), out_cap=d_out.numel(), **cut)
    on_host = lambda: ix.tally_lines(stream, table, limit=TOP)
    if a.one_call:
        r = on_device()
        print(json.dumps({"n_lines": r.n_lines, "n_distinct": r.n_distinct}))
        return

    def counter_in_python():
        lines = np.asarray(pkg.Bzip2.decompressFile(stream)).tobytes().split(b"\n")
        if not lines[-1]:
            lines.pop()
        first = {}
        for k, ln in enumerate(lines):
            first.setdefault(ln, k)
        c = collections.Counter(lines)
        top = sorted(c.items(), key=lambda kv: (-kv[1], first[kv[0]]))[:TOP]
        return len(lines), len(c), [(first[ln], cnt) for ln, cnt in top]

    def unique_on_host(keys):
        _, first, counts = np.unique(keys, return_index=True, return_counts=True)
        order = np.lexsort((first, -counts))[:TOP]
        return int(first.size), [(int(first[i]), int(counts[i])) for i in order]

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    pairs = lambda r: [(int(g["first"]), int(g["count"])) for g in r.groups]
    # results first
    n_lines, n_distinct, top = counter_in_python()
    keys, _ = pkg.line_keys_device(ptr, n, ix, table)
    if keys.size and keys[-1].tolist() == (0, 0, 0):
        keys = keys[:-1]                                    # the empty tail is no line (only it has length 0: every other line holds its newline)
    for r in (on_device(), on_host()):
        assert (r.n_lines, r.n_bad_lines, r.n_distinct, r.n_groups) == (n_lines, 0, n_distinct, n_distinct) and pairs(r) == top, "a tally differs from the Counter"
    text = data.tobytes()
    for name, cut in CUTS.items():                            # the tally of a cut against the Counter over cut_text's lines
        lines = pkg.cut_text(text, **cut).split(b"\n")[:-1]
        first = {}
        for k, ln in enumerate(lines):
            first.setdefault(ln, k)
        c = collections.Counter(lines)
        want = [(first[ln], cnt) for ln, cnt in sorted(c.items(), key=lambda kv: (-kv[1], first[kv[0]]))[:TOP]]
        r = on_device(**cut)
        assert (r.n_lines, r.n_distinct) == (len(lines), len(c)) and pairs(r) == want, "the tally of a cut differs from the Counter (%s)" % name
    r = pkg.tally_keys(keys, limit=TOP)                      # (a tail without a newline has a key of its own here: held against numpy, not the Counter)
    assert unique_on_host(keys) == (r.n_distinct, pairs(r)) and r.n_lines == keys.size, "tally_keys differs from numpy.unique"
    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": ix.blocks, "lines": n_lines, "distinct": n_distinct,
                      "top": top[:3]}))
    groups = {"device": {"line_keys_device": lambda: pkg.line_keys_device(ptr, n, ix, table), "tally_lines_device": on_device,
                         **{"cut_lines_device " + k: (lambda cut=cut: cut_device(**cut)) for k, cut in CUTS.items()},
                         **{"tally_lines_device " + k: (lambda cut=cut: on_device(**cut)) for k, cut in CUTS.items()}},
              "host": {"decompress_then_counter_in_python": counter_in_python, "tally_lines": on_host},
              "keys": {"numpy_unique": lambda: unique_on_host(keys), "tally_keys": lambda: pkg.tally_keys(keys, limit=TOP)}}
    slow = ("decompress_then_counter_in_python",)
    for name, ways in groups.items():
        for wname, f in ways.items():
            if wname not in slow:
                f()                                         # warm-up
        ts = {wname: [] for wname in ways}
        for i in range(a.reps):
            for wname, f in ways.items():
                if wname not in slow or i == 0:
                    ts[wname].append(ms(f))
        print(json.dumps({"group": name, **{wname: stats(v) for wname, v in ts.items()}}))


if __name__ == "__main__":
    main()
