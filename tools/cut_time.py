#!/usr/bin/env python3
"""The column cut of a .bz2 stream against what it rides on and what a user does without it, every result checked before anything
is timed.  One JSON line per group.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1), its index and its line table; the delimiter is b" ".
  device   cut_lines_device of the whole stream (stream and result in HBM) with fields 1, 2-3, 1- and with bytes 1-16   against
           read_ranges_device of the whole stream (the same decode plus a copy) and lines_build_device (the same decode plus one
           light pass over the same tiles): the yardsticks
  host     Bzip2Index.cut_lines (the result in host memory) with the same selections   against  cjs_bzip2_decompress plus a split
           into lines and fields in Python (fields 1; one run)
The ways alternate in one process after a warm-up of each: median and spread (max - min) of --reps runs.  Every output is first
compared with cut_text (the library's scalar walk over the plain text).  The H2D / D2H bytes come from the library's "[cjs cut]"
lines (CJS_DEBUG), collected by a child process of this tool that makes each call once, under a time limit; if the child fails or
runs into the limit, the tool stops before it opens the GPU.

--one-call makes one cut_lines_device call of the whole stream (fields 2-3) and nothing else: the program for a kernel trace of its
own,
  rocprofv3 --kernel-trace --stats --output-format csv -d tool_out/cut_trace -- python tools/cut_time.py [MB] --one-call
whose stats give the share of ct_summary / ct_chain / ct_count / ct_scan / ct_emit in the call.

usage: python tools/cut_time.py [MB] [--reps 5]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SELECTIONS = (("fields", "1"), ("fields", "2-3"), ("fields", "1-"), ("bytes", "1-16"))
DELIM = b" "
N_DEBUG = 2 * len(SELECTIONS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", action="store_true", help="one cut_lines_device call of the whole stream and nothing else")
    ap.add_argument("--debug-lines", action="store_true", help="(the child) one call of each kind under CJS_DEBUG")
    ap.add_argument("--child-timeout", type=int, default=0, help="seconds for that child (default: by the input size)")
    a = ap.parse_args()
    nbytes = a.mb * 1000000
    debug = []
    if not a.debug_lines and not a.one_call:                # before this process opens the GPU
        # The child runs under a time limit, and anything but a clean end with its lines stops the tool here: nothing more is
        # started on a GPU that a process has just faulted or hung on.
        limit = a.child_timeout or 120 + 3 * a.mb
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(a.mb), "--debug-lines"]
        child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, CJS_DEBUG="1"))
        debug = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs cut]")]
        if child.returncode != 0 or len(debug) != N_DEBUG:
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("cut_time: the CJS_DEBUG child ended with status %d and %d of %d '[cjs cut]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(debug), N_DEBUG, limit))
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    ix = pkg.Bzip2Index.build(stream)
    d_in = torch.from_numpy(stream).cuda()
    d_out = torch.empty(data.size + 1, dtype=torch.uint8, device="cuda")       # the window's bytes + 1 are always enough
    torch.cuda.synchronize()
    ptr, n = d_in.data_ptr(), stream.size
    table = pkg.lines_build_device(ptr, n, ix)
    on_device = lambda kind, spec: pkg.cut_lines_device(ptr, n, ix, table, delimiter=DELIM, d_out_ptr=d_out.data_ptr(), out_cap=d_out.numel(), **{kind: spec})
    on_host = lambda kind, spec: ix.cut_lines(stream, table, delimiter=DELIM, **{kind: spec})
    if a.one_call:
        print(json.dumps({"out_bytes": on_device("fields", "2-3")}))
        return
    if a.debug_lines:
        for kind, spec in SELECTIONS:
            on_device(kind, spec)
            on_host(kind, spec)
        return

    def split_in_python():
        text = np.asarray(pkg.Bzip2.decompressFile(stream)).tobytes()
        lines = text.split(b"\n")
        if not lines[-1]:
            lines.pop()
        return b"".join(ln.split(DELIM, 1)[0] + b"\n" for ln in lines)

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    floor = lambda: pkg.read_ranges_device(ptr, n, ix, [(0, data.size)], d_out.data_ptr(), d_out.numel())
    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": ix.blocks, "newlines": int((data == 10).sum())}))
    # results first
    sizes = {}
    for kind, spec in SELECTIONS:
        want = pkg.cut_text(data, delimiter=DELIM, **{kind: spec})
        got = on_device(kind, spec)
        assert got == len(want) and d_out[:got].cpu().numpy().tobytes() == want, "the device form differs from cut_text (%s %s)" % (kind, spec)
        assert on_host(kind, spec) == want, "the host form differs from cut_text (%s %s)" % (kind, spec)
        sizes["%s %s" % (kind, spec)] = len(want)
    assert split_in_python() == pkg.cut_text(data, delimiter=DELIM, fields="1")
    floor()
    assert np.array_equal(d_out[:data.size].cpu().numpy(), data)
    groups = {"device": {"read_ranges_device_whole": floor, "lines_build_device": lambda: pkg.lines_build_device(ptr, n, ix).counts()},
              "host": {"decompress_then_split_in_python": split_in_python}}
    for kind, spec in SELECTIONS:
        groups["device"]["cut_lines_device %s %s" % (kind, spec)] = lambda kind=kind, spec=spec: on_device(kind, spec)
        groups["host"]["cut_lines %s %s" % (kind, spec)] = lambda kind=kind, spec=spec: on_host(kind, spec)
    slow = ("decompress_then_split_in_python",)
    for name, ways in groups.items():
        for wname, f in ways.items():
            if wname not in slow:
                f()                                         # warm-up
        ts = {wname: [] for wname in ways}
        for i in range(a.reps):
            for wname, f in ways.items():
                if wname not in slow or i == 0:
                    ts[wname].append(ms(f))
        row = {"group": name, **{wname: stats(v) for wname, v in ts.items()}, "out_bytes": sizes}
        row["debug"] = debug[0::2] if name == "device" else debug[1::2]
        print(json.dumps(row))


if __name__ == "__main__":
    main()
