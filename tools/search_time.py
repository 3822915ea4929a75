#!/usr/bin/env python3
"""Pattern search in a .bz2 stream against the ways to the same list without it, every list checked before anything is timed.
One JSON line per pattern set.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes) and its index.  Pattern sets, cut from the text:
one 8-byte pattern, 16 patterns, 64 patterns (lengths 8..64).
  host form    cjs_bzip2_search                against  cjs_bzip2_decompress followed by the same search on the CPU (bytes.find)
  device form  search_device (stream in HBM)   against  decompress_device (the decode alone: no search at all), and against
                                               read_ranges_device of the whole stream (the same engine, the gather for the scan)
alternating in one process after a warm-up of each: median and spread (max - min) of --reps runs (the CPU search: 1 run).  The
H2D / D2H bytes come from the library's "[cjs search]" lines (CJS_DEBUG), collected by a child process of this tool that makes
each call once, under a time limit; if the child fails or runs into the limit, the tool stops before it opens the GPU.

--one-call N makes one device-form search with the N-pattern set and nothing else: the program for a kernel trace of its own,
  rocprofv3 --kernel-trace --stats -d tool_out/search_trace -- python tools/search_time.py [MB] --one-call 64
whose stats give the share of sr_count / sr_scan / sr_emit in the call.

usage: python tools/search_time.py [MB] [--big] [--reps 5]
"""
import argparse
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


def pattern_sets(data):
    rng = np.random.RandomState(11)
    sets = {}
    for count in (1, 16, 64):
        lens = [8] if count == 1 else [int(x) for x in rng.randint(8, 65, count)]
        sets[count] = [data[s:s + n].tobytes() for s, n in zip(rng.randint(0, data.size - 64, count), lens)]
    return sets


def cpu_search(text, pats):
    out = []
    for j, p in enumerate(pats):
        at = text.find(p)
        while at >= 0:
            out.append((at, j))
            at = text.find(p, at + 1)
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", type=int, default=0, help="one device-form search with this pattern set (1, 16 or 64) and nothing else")
    ap.add_argument("--debug-lines", action="store_true", help="(the child) one call per set and form under CJS_DEBUG")
    ap.add_argument("--child-timeout", type=int, default=0, help="seconds for that child (default: by the input size)")
    a = ap.parse_args()
    nbytes = 1 << 30 if a.big else a.mb * 1000000
    debug = []
    if not a.debug_lines and not a.one_call:                # before this process opens the GPU
        # The child runs under a time limit, and anything but a clean end with its six lines stops the tool here: nothing more is
        # started on a GPU that a process has just faulted or hung on.
        limit = a.child_timeout or (1200 if a.big else 120 + 3 * a.mb)
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(a.mb), "--debug-lines"] + (["--big"] if a.big else [])
        child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, CJS_DEBUG="1"))
        debug = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs search]")]
        if child.returncode != 0 or len(debug) != 6:
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("search_time: the CJS_DEBUG child ended with status %d and %d of 6 '[cjs search]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(debug), limit))
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    ix = pkg.Bzip2Index.build(stream)
    sets = pattern_sets(data)
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    if a.one_call:
        res = pkg.search_device(d_in.data_ptr(), stream.size, ix, sets[a.one_call], limit=1 << 20)
        print(json.dumps({"patterns": a.one_call, "total": res.total}))
        return
    if a.debug_lines:
        for count in (1, 16, 64):
            ix.search(stream, sets[count], limit=1 << 20)
            pkg.search_device(d_in.data_ptr(), stream.size, ix, sets[count], limit=1 << 20)
        return
    d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    text = data.tobytes()

    ways = {
        "search_host": lambda pats: ix.search(stream, pats, limit=1 << 20).matches,
        "decompress_then_cpu": lambda pats: cpu_search(pkg.Bzip2.decompressFile(stream).tobytes(), pats),
        "search_device": lambda pats: pkg.search_device(d_in.data_ptr(), stream.size, ix, pats, limit=1 << 20).matches,
        "decompress_device": lambda pats: pkg.decompress_device(d_in.data_ptr(), stream.size, d_full.data_ptr(), d_full.numel()),
        "read_ranges_device": lambda pats: pkg.read_ranges_device(d_in.data_ptr(), stream.size, ix, [(0, data.size)], d_full.data_ptr(), d_full.numel()),
    }

    def ms(f, pats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f(pats)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": ix.blocks}))
    for k, count in enumerate((1, 16, 64)):
        pats = sets[count]
        want = cpu_search(text, pats)                       # results first
        assert len(want) < 1 << 20
        assert ways["search_host"](pats) == want and ways["search_device"](pats) == want, count
        for name in ("decompress_device", "read_ranges_device"):      # (their warm-up; the bytes are the range tests' business)
            ways[name](pats)
        assert np.array_equal(d_full.cpu().numpy(), data)
        ts = {name: [] for name in ways}
        for i in range(a.reps):
            for name, f in ways.items():
                if name != "decompress_then_cpu" or i == 0:
                    ts[name].append(ms(f, pats))
        print(json.dumps({"patterns": count, "matches": len(want), **{name: stats(v) for name, v in ts.items()},
                          "debug_host": debug[2 * k] if debug else "", "debug_device": debug[2 * k + 1] if debug else ""}))


if __name__ == "__main__":
    main()
