#!/usr/bin/env python3
"""Regex search in a .bz2 stream against the literal search and against the ways to the same list without it, every list checked
before anything is timed.  One JSON line per operating point.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes) and its index.  Operating points:
  lit1, lit16, lit64   the 1, 16 and 64 literal patterns of tools/search_time.py written as regexes (re.escape).  A set whose tables
                       do not fit CJS_REGEX_MAX_TABLE_BYTES is reported as refused, with the library's text, and its longest prefix
                       that fits is timed in its place ("patterns" says how many that is)
  digits               \\d{4}
  names                [A-Z][a-z]{2,10} [A-Z][a-z]+
  alert                [Ee]rror|[Ww]arn(ing)?
  worst                .{0,200}x     (the worst case by design: every position walks its line)
  device form  search_regex_device  against  search_device on the same patterns (the literal points only) and read_ranges_device of
                                             the whole stream (the same engine, the gather for the scan)
  host form    search_regex         against  cjs_bzip2_decompress followed by re.finditer on the CPU
alternating in one process after a warm-up of each: median and spread (max - min) of --reps runs (the CPU way: 1 run).
The lists are checked first: over the whole stream the host form against the device form and the literal points against
search_device with the patterns' lengths; over the first --scan-bytes of the text the start offsets of every pattern against `re`
(a lookahead scan, which finds overlapping starts); over the first --check-bytes offsets and lengths against the per-position
oracle of the tests (tests/regex_cases.expected).  Python's `re` is what bounds the two prefixes: the worst-case point costs it
about 200 steps per position.  The H2D / D2H bytes come from the library's "[cjs regex]" lines (CJS_DEBUG), collected by a child
process of this tool that makes each call once, under a time limit; if the child fails or runs into the limit, the tool stops
before it opens the GPU.

--one-call POINT makes one device-form regex search at that point and nothing else: the program for a kernel trace of its own,
  rocprofv3 --kernel-trace --stats -d tool_out/regex_trace -- python tools/regex_time.py [MB] --one-call digits
whose stats give the share of rx_count / sr_scan / rx_emit in the call.

usage: python tools/regex_time.py [MB] [--big] [--reps 5] [--scan-bytes 5000000] [--check-bytes 100000]
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT = 1 << 20
POINTS = ("lit1", "lit16", "lit64", "digits", "names", "alert", "worst")
FIXED = {"digits": [rb"\d{4}"], "names": [rb"[A-Z][a-z]{2,10} [A-Z][a-z]+"], "alert": [rb"[Ee]rror|[Ww]arn(ing)?"], "worst": [rb".{0,200}x"]}


def points(pkg, data):
    """name -> (regexes, the literals behind them or None, the refusal of the whole set or None)"""
    import search_time
    sets = search_time.pattern_sets(data)
    out = {}
    for count in (1, 16, 64):
        lits, refusal = list(sets[count]), None
        while True:
            try:
                pkg.regex_check([re.escape(p) for p in lits])
                break
            except pkg.CjsError as e:
                refusal = refusal or str(e)
                lits.pop()
        out["lit%d" % count] = ([re.escape(p) for p in lits], lits, refusal)
    for name, pats in FIXED.items():
        out[name] = (pats, None, None)
    return out


def starts_by_re(text, pats):
    """per pattern the sorted offsets at which a match starts (overlapping ones too), by a lookahead scan"""
    return [[m.start() for m in re.finditer(b"(?=(?:" + p + b"))", text)] for p in pats]


def finditer_all(text, pats):
    return sum(sum(1 for _ in re.finditer(p, text)) for p in pats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scan-bytes", type=int, default=5000000, help="the prefix of the text over which the start offsets are checked against re")
    ap.add_argument("--check-bytes", type=int, default=100000, help="the prefix of the text over which the lengths are checked per position")
    ap.add_argument("--one-call", default="", help="one device-form regex search at this point (%s) and nothing else" % ", ".join(POINTS))
    ap.add_argument("--debug-lines", action="store_true", help="(the child) one call per point and form under CJS_DEBUG")
    ap.add_argument("--child-timeout", type=int, default=0, help="seconds for that child (default: by the input size)")
    a = ap.parse_args()
    nbytes = 1 << 30 if a.big else a.mb * 1000000
    debug = []
    if not a.debug_lines and not a.one_call:                # before this process opens the GPU
        # The child runs under a time limit, and anything but a clean end with its lines stops the tool here: nothing more is
        # started on a GPU that a process has just faulted or hung on.
        limit = a.child_timeout or (1200 if a.big else 120 + 4 * a.mb)
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(a.mb), "--debug-lines"] + (["--big"] if a.big else [])
        child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, CJS_DEBUG="1"))
        debug = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs regex]")]
        if child.returncode != 0 or len(debug) != 2 * len(POINTS):
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("regex_time: the CJS_DEBUG child ended with status %d and %d of %d '[cjs regex]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(debug), 2 * len(POINTS), limit))
    import torch
    import recipes
    import regex_cases
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    ix = pkg.Bzip2Index.build(stream)
    pts = points(pkg, data)
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    if a.one_call:
        res = pkg.search_regex_device(d_in.data_ptr(), stream.size, ix, pts[a.one_call][0], limit=LIMIT)
        print(json.dumps({"point": a.one_call, "patterns": len(pts[a.one_call][0]), "total": res.total}))
        return
    if a.debug_lines:
        for name in POINTS:
            ix.search_regex(stream, pts[name][0], limit=LIMIT)
            pkg.search_regex_device(d_in.data_ptr(), stream.size, ix, pts[name][0], limit=LIMIT)
        return
    d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    text = data.tobytes()

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": ix.blocks}))
    for k, name in enumerate(POINTS):
        pats, lits, refusal = pts[name]
        ways = {
            "search_regex_host": lambda: ix.search_regex(stream, pats, limit=LIMIT),
            "decompress_then_re": lambda: finditer_all(pkg.Bzip2.decompressFile(stream).tobytes(), pats),
            "search_regex_device": lambda: pkg.search_regex_device(d_in.data_ptr(), stream.size, ix, pats, limit=LIMIT),
            "read_ranges_device": lambda: pkg.read_ranges_device(d_in.data_ptr(), stream.size, ix, [(0, data.size)], d_full.data_ptr(), d_full.numel()),
        }
        if lits:
            ways["search_device"] = lambda: pkg.search_device(d_in.data_ptr(), stream.size, ix, lits, limit=LIMIT)
        # results first
        host, dev = ways["search_regex_host"](), ways["search_regex_device"]()
        assert host.matches == dev.matches and host.total == dev.total, name
        scan = min(a.scan_bytes, data.size)
        starts = starts_by_re(text[:scan], pats)
        part = pkg.search_regex_device(d_in.data_ptr(), stream.size, ix, pats, length=scan, limit=None)
        assert [(o, j) for o, j, n in part.matches] == sorted((o, j) for j, s in enumerate(starts) for o in s), name
        head = pkg.search_regex_device(d_in.data_ptr(), stream.size, ix, pats, length=a.check_bytes, limit=None)
        assert head.matches == regex_cases.expected(data[:a.check_bytes], pats), name
        if lits:
            lit = ways["search_device"]()
            assert [(o, j, len(lits[j])) for o, j in lit.matches] == dev.matches and lit.total == dev.total, name
        ways["read_ranges_device"]()                        # (its warm-up; the bytes are the range tests' business)
        ts = {w: [] for w in ways}
        for i in range(a.reps):
            for w, f in ways.items():
                if w != "decompress_then_re" or i == 0:
                    ts[w].append(ms(f))
        print(json.dumps({"point": name, "regexes": [p.decode("latin1") for p in pats][:4], "patterns": len(pats), "refused_whole_set": refusal, "matches": dev.total,
                          **{w: stats(v) for w, v in ts.items()}, "debug_host": debug[2 * k] if debug else "", "debug_device": debug[2 * k + 1] if debug else ""}), flush=True)


if __name__ == "__main__":
    main()
