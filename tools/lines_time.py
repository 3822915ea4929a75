#!/usr/bin/env python3
"""The line table of a .bz2 stream against what a user does without it, every result checked before anything is timed.  One JSON
line per question.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes), its index and its line table.
  build        lines_build_device (stream in HBM)    against  search_device with the one pattern b"\\n" as a count query
  locate       line_starts_device, 1 and 10,000 random line numbers     against  cjs_bzip2_decompress plus numpy on the host
  number       line_numbers_device, 1 and 10,000 random offsets         against  the same
  grep_lines   Bzip2Index.grep_lines with the 16-pattern set of search_time.py   against  the same, plus bytes.find
and everything against read_ranges_device of the whole stream, the decode floor of the engine.  The ways alternate in one process
after a warm-up of each: median and spread (max - min) of --reps runs (the host ways: 1 run).  The H2D / D2H bytes come from the
library's "[cjs lines]" lines (CJS_DEBUG), collected by a child process of this tool that makes each call once, under a time
limit; if the child fails or runs into the limit, the tool stops before it opens the GPU.

--one-call makes one build, one locate and one number call of 10,000 questions (device form) and nothing else: the program for a
kernel trace of its own,
  rocprofv3 --kernel-trace --stats -d tool_out/lines_trace -- python tools/lines_time.py [MB] --one-call
whose stats give the share of ln_count / ln_scan / ln_select / ln_rank in the calls.

usage: python tools/lines_time.py [MB] [--big] [--reps 5]
"""
import argparse
import bisect
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_DEBUG = 5


def questions(nl, total):
    rng = np.random.RandomState(21)
    lines = rng.randint(1, nl.size + 1, 10000).astype(np.uint64)
    offsets = rng.randint(1, total, 10000).astype(np.uint64)
    return lines, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", action="store_true", help="one build, one locate and one number call (device form) and nothing else")
    ap.add_argument("--debug-lines", action="store_true", help="(the child) one call of each kind under CJS_DEBUG")
    ap.add_argument("--child-timeout", type=int, default=0, help="seconds for that child (default: by the input size)")
    a = ap.parse_args()
    nbytes = 1 << 30 if a.big else a.mb * 1000000
    debug = []
    if not a.debug_lines and not a.one_call:                # before this process opens the GPU
        # The child runs under a time limit, and anything but a clean end with its lines stops the tool here: nothing more is
        # started on a GPU that a process has just faulted or hung on.
        limit = a.child_timeout or (1200 if a.big else 120 + 3 * a.mb)
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(a.mb), "--debug-lines"] + (["--big"] if a.big else [])
        child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, CJS_DEBUG="1"))
        debug = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs lines]")]
        if child.returncode != 0 or len(debug) != N_DEBUG:
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("lines_time: the CJS_DEBUG child ended with status %d and %d of %d '[cjs lines]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(debug), N_DEBUG, limit))
    import torch
    import recipes
    import search_time
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    ix = pkg.Bzip2Index.build(stream)
    total = int(data.size)
    nl = np.flatnonzero(data == 10)
    lines, offsets = questions(nl, total)
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    ptr, n = d_in.data_ptr(), stream.size
    table = pkg.lines_build_device(ptr, n, ix)
    if a.one_call or a.debug_lines:
        pkg.line_starts_device(ptr, n, ix, table, lines[:1] if a.debug_lines else lines)
        if a.debug_lines:
            pkg.line_starts_device(ptr, n, ix, table, lines)
            pkg.line_numbers_device(ptr, n, ix, table, offsets[:1])
        pkg.line_numbers_device(ptr, n, ix, table, offsets)
        if a.one_call:
            print(json.dumps({"newlines": table.newlines}))
        return
    d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    pats = search_time.pattern_sets(data)[16]

    def host_plain():
        return np.asarray(pkg.Bzip2.decompressFile(stream))

    def host_starts(q):
        at = np.flatnonzero(host_plain() == 10)
        return at[q.astype(np.int64) - 1] + 1

    def host_numbers(q):
        at = np.flatnonzero(host_plain() == 10)
        return np.searchsorted(at, q.astype(np.int64), "left")

    def host_grep():
        text = host_plain().tobytes()
        found = search_time.cpu_search(text, pats)
        text_lines = text.splitlines(keepends=True)
        starts = np.concatenate([[0], np.cumsum([len(x) for x in text_lines])]).tolist()
        by = {}
        for o, j in found:
            by.setdefault(bisect.bisect_right(starts, o) - 1, []).append((o, j))
        return [(no, text_lines[no], m) for no, m in sorted(by.items())]

    groups = {
        "build": {
            "lines_build_device": lambda: pkg.lines_build_device(ptr, n, ix).counts(),
            "search_count_newline": lambda: pkg.search_device(ptr, n, ix, [b"\n"], limit=0).total,
        },
        "locate_1": {"line_starts_device": lambda: pkg.line_starts_device(ptr, n, ix, table, lines[:1])[0], "decompress_then_numpy": lambda: host_starts(lines[:1])},
        "locate_10000": {"line_starts_device": lambda: pkg.line_starts_device(ptr, n, ix, table, lines)[0], "decompress_then_numpy": lambda: host_starts(lines)},
        "number_1": {"line_numbers_device": lambda: pkg.line_numbers_device(ptr, n, ix, table, offsets[:1])[0], "decompress_then_numpy": lambda: host_numbers(offsets[:1])},
        "number_10000": {"line_numbers_device": lambda: pkg.line_numbers_device(ptr, n, ix, table, offsets)[0], "decompress_then_numpy": lambda: host_numbers(offsets)},
        "grep_lines_16": {"grep_lines": lambda: ix.grep_lines(stream, table, pats), "decompress_then_cpu": host_grep},
    }
    floor = lambda: pkg.read_ranges_device(ptr, n, ix, [(0, data.size)], d_full.data_ptr(), d_full.numel())

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    print(json.dumps({"input_bytes": total, "stream_bytes": int(stream.size), "blocks": ix.blocks, "newlines": int(nl.size)}))
    # results first
    want_counts = [int(c) for c in np.diff(np.searchsorted(nl, np.concatenate([[0], np.cumsum([e[2] for e in ix.entries()])])))]
    assert table.counts().tolist() == want_counts and groups["build"]["search_count_newline"]() == nl.size == table.newlines
    assert groups["locate_10000"]["line_starts_device"]().tolist() == (nl[lines.astype(np.int64) - 1] + 1).tolist()
    assert groups["number_10000"]["line_numbers_device"]().tolist() == np.searchsorted(nl, offsets.astype(np.int64), "left").tolist()
    assert groups["grep_lines_16"]["grep_lines"]() == host_grep()
    floor()
    assert np.array_equal(d_full.cpu().numpy(), data)
    slow = ("decompress_then_numpy", "decompress_then_cpu")
    for k, (name, ways) in enumerate(groups.items()):
        ways = dict(ways, read_ranges_device_whole=floor)
        for wname, f in ways.items():
            if wname not in slow:
                f()                                         # warm-up
        ts = {wname: [] for wname in ways}
        for i in range(a.reps):
            for wname, f in ways.items():
                if wname not in slow or i == 0:
                    ts[wname].append(ms(f))
        print(json.dumps({"question": name, **{wname: stats(v) for wname, v in ts.items()}, "debug": debug[k] if k < len(debug) else ""}))


if __name__ == "__main__":
    main()
