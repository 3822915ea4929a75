#!/usr/bin/env python3
"""The line sort of a .bz2 stream against what it rides on and what a user does without it, every result checked against Python's
sorted() over the real lines before anything is timed.  One JSON line per group.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1), its index and its line table.
  device   sort_lines_device of the whole stream in five forms: whole lines; limit=10; unique; whole lines with the text; bytes 1-16
           against   cut_lines_device with bytes 1- (the same decode and the same text: what the sort costs beyond it),
           tally_lines_device (limit=10) and read_ranges_device of the whole stream: the yardsticks
  host     Bzip2Index.sort_lines (the stream in host memory)   against   cjs_bzip2_decompress plus sorted() in Python (one run)
The ways alternate in one process after a warm-up of each: median and spread (max - min) of --reps runs.

--one-call makes one sort_lines_device call of the whole stream and nothing else: the program for a kernel trace of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -d tool_out/sort_trace -- python tools/sort_time.py [MB] --one-call
whose stats give the share of the radix passes, of sl_words' gathered reads and of the other sl_* kernels in the call.

usage: python tools/sort_time.py [MB] [--reps 5]
"""
import argparse
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
    ap.add_argument("--one-call", action="store_true", help="one sort_lines_device call of the whole stream and nothing else")
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
    d_out = torch.empty(data.size + 1, dtype=torch.uint8, device="cuda")
    out = dict(d_text_out_ptr=d_out.data_ptr(), text_cap=d_out.numel())
    on_device = lambda **kw: pkg.sort_lines_device(ptr, n, ix, table, **kw)
    if a.one_call:
        r = on_device()
        print(json.dumps({"n_lines": r.n_lines, "n_distinct": r.n_distinct, "rounds": r.rounds}))
        return
    FORMS = {"whole lines": {}, "limit 10": dict(limit=TOP), "unique": dict(unique=True), "whole lines with text": dict(out),
             "bytes 1-16": dict(bytes="1-16")}
    cut_device = lambda: pkg.cut_lines_device(ptr, n, ix, table, bytes="1-", d_out_ptr=d_out.data_ptr(), out_cap=d_out.numel())
    on_host = lambda: ix.sort_lines(stream, table)

    def sorted_in_python():
        lines = np.asarray(pkg.Bzip2.decompressFile(stream)).tobytes().split(b"\n")
        if not lines[-1]:
            lines.pop()
        return lines, sorted(range(len(lines)), key=lambda i: (lines[i], i))

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    # results first
    lines, order = sorted_in_python()
    firsts = [order[k] for k in range(len(order)) if k == 0 or lines[order[k]] != lines[order[k - 1]]]
    r = on_device()
    assert (r.n_lines, r.n_out, r.n_distinct) == (len(lines), len(lines), len(firsts)) and r.lines.tolist() == order, "the sort differs from sorted()"
    rounds = r.rounds
    assert on_host().lines.tolist() == order, "the host form differs from sorted()"
    assert on_device(limit=TOP).lines.tolist() == order[:TOP]
    u = on_device(unique=True)
    assert u.lines.tolist() == firsts and int(u.counts.sum()) == len(lines), "sort -u differs"
    t = on_device(**out)
    assert d_out[:t.text_n].cpu().numpy().tobytes() == b"".join(lines[i] + b"\n" for i in order), "the sorted text differs"
    cut16 = [x[:16] for x in lines]
    assert on_device(bytes="1-16").lines.tolist() == sorted(range(len(lines)), key=lambda i: (cut16[i], i)), "the sort of a cut differs"
    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": ix.blocks, "lines": len(lines), "distinct": len(firsts),
                      "rounds": rounds, "longest_line": max(map(len, lines))}))
    whole = [(0, int(data.size))]
    groups = {"device": {"cut_lines_device bytes 1-": cut_device, "tally_lines_device": lambda: pkg.tally_lines_device(ptr, n, ix, table, limit=TOP),
                         "read_ranges_device": lambda: pkg.read_ranges_device(ptr, n, ix, whole, d_out.data_ptr(), d_out.numel()),
                         **{"sort_lines_device " + k: (lambda kw=kw: on_device(**kw)) for k, kw in FORMS.items()}},
              "host": {"decompress_then_sorted_in_python": sorted_in_python, "sort_lines": on_host}}
    slow = ("decompress_then_sorted_in_python",)
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
