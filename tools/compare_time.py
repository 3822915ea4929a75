#!/usr/bin/env python3
"""Compare of a .bz2 stream against the ways to the same answer without it, every answer checked before anything is timed.
One JSON line per case.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes) and its index; the other side is the plain text:
equal, with one byte flipped, with 1 % of its bytes flipped.
  device form  compare_device (stream and text in HBM)  against  decompress_device into a second buffer + torch.equal, against
                                                        read_ranges_device of the whole stream (the same engine, the gather
                                                        for the compare) and against a device copy of the same bytes
  host form    Bzip2Index.compare                       against  cjs_bzip2_decompress + numpy.array_equal
  two streams  compare_streams_device, the level-1      against  two decompress_device calls + torch.equal
               stream of the text against the level-9
alternating in one process after a warm-up of each: median and spread (max - min) of --reps runs.  peak_bytes is the most device
memory in use during one more run of each way beyond what was in use before it (the free memory sampled by a thread; the inputs
and the baselines' result buffers are allocated inside the run, so they count).  The H2D / D2H bytes come from the library's
"[cjs compare]" lines (CJS_DEBUG), collected by a child process of this tool that makes each call once, under a time limit; if
the child fails or runs into the limit, the tool stops before it opens the GPU.

--one-call CASE makes one device-form compare (equal, one or percent) and nothing else: the program for a kernel trace of its own,
  rocprofv3 --kernel-trace --stats -d tool_out/compare_trace -- python tools/compare_time.py [MB] --one-call equal
whose stats give the share of cm_count / cm_scan / cm_emit in the call.

usage: python tools/compare_time.py [MB] [--big] [--reps 5]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("equal", "one", "percent")
DEBUG_LINES = 5


def others(data):
    """the other side of every case: the text, one byte flipped in the middle, 1 % of the bytes flipped"""
    one = data.copy()
    one[data.size // 2] ^= 0x20
    pct = data.copy()
    at = np.unique(np.random.RandomState(3).randint(0, data.size, data.size // 100))
    pct[at] ^= 0xFF
    return {"equal": data, "one": one, "percent": pct}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", choices=CASES, help="one device-form compare of this case and nothing else")
    ap.add_argument("--debug-lines", action="store_true", help="(the child) one call per case and form under CJS_DEBUG")
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
        debug = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs compare]")]
        if child.returncode != 0 or len(debug) != DEBUG_LINES:
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("compare_time: the CJS_DEBUG child ended with status %d and %d of %d '[cjs compare]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(debug), DEBUG_LINES, limit))
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    side = others(data)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    ix = pkg.Bzip2Index.build(stream)
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    if a.one_call:
        pkg.trim()
        d_other = torch.from_numpy(side[a.one_call]).cuda()
        torch.cuda.synchronize()
        res = pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_other.data_ptr(), data.size)
        print(json.dumps({"case": a.one_call, "total": res.total, "compared": res.compared}))
        return
    stream1 = np.array(pkg.Bzip2.compressFile(data, None, 1))
    pkg.trim()
    ix1 = pkg.Bzip2Index.build(stream1)
    d_in1 = torch.from_numpy(stream1).cuda()
    d_side = {c: torch.from_numpy(side[c]).cuda() for c in CASES}
    torch.cuda.synchronize()
    if a.debug_lines:
        for c in CASES:
            pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_side[c].data_ptr(), data.size)
        ix.compare(stream, data)
        pkg.compare_streams_device(d_in1.data_ptr(), stream1.size, ix1, d_in.data_ptr(), stream.size, ix)
        return

    def decode_equal(d_other):
        d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
        pkg.decompress_device(d_in.data_ptr(), stream.size, d_full.data_ptr(), d_full.numel())
        return bool(torch.equal(d_full, d_other))

    def two_decodes_equal():
        x, y = torch.empty(data.size, dtype=torch.uint8, device="cuda"), torch.empty(data.size, dtype=torch.uint8, device="cuda")
        pkg.decompress_device(d_in1.data_ptr(), stream1.size, x.data_ptr(), x.numel())
        pkg.decompress_device(d_in.data_ptr(), stream.size, y.data_ptr(), y.numel())
        return bool(torch.equal(x, y))

    def whole_range():
        d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
        pkg.read_ranges_device(d_in.data_ptr(), stream.size, ix, [(0, data.size)], d_full.data_ptr(), d_full.numel())
        return d_full

    def device_copy(d_other):
        d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
        d_full.copy_(d_other)
        return d_full

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def peak(f):
        """device bytes in use during f() beyond those in use before it"""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        low, stop = [free0], threading.Event()

        def watch():
            while not stop.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info()[0])
                time.sleep(0.0005)
        t = threading.Thread(target=watch)
        t.start()
        f()
        torch.cuda.synchronize()
        low[0] = min(low[0], torch.cuda.mem_get_info()[0])
        stop.set()
        t.join()
        return int(free0 - low[0])

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    def measure(ways):
        for f in ways.values():                             # warm-up
            f()
        ts = {name: [] for name in ways}
        for i in range(a.reps):
            for name, f in ways.items():
                ts[name].append(ms(f))
        out = {name: stats(v) for name, v in ts.items()}
        for name, f in ways.items():
            pkg.trim()
            out[name]["peak_bytes"] = peak(f)
        return out

    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": ix.blocks, "level1_stream_bytes": int(stream1.size), "level1_blocks": ix1.blocks}))
    for k, c in enumerate(CASES):
        want = np.nonzero(data != side[c])[0]               # results first
        res = pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_side[c].data_ptr(), data.size, limit=64)
        assert res.total == want.size and res.compared == data.size and [d[0] for d in res.diffs] == want[:64].tolist() and res.equal == (want.size == 0), c
        assert decode_equal(d_side[c]) == (want.size == 0) and bool(torch.equal(whole_range(), d_side["equal"]))
        ways = {
            "compare_device": lambda: pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_side[c].data_ptr(), data.size, limit=64),
            "compare_device_count": lambda: pkg.compare_device(d_in.data_ptr(), stream.size, ix, d_side[c].data_ptr(), data.size, limit=0),
            "decompress_device_then_equal": lambda: decode_equal(d_side[c]),
            "read_ranges_device": whole_range,
            "device_copy": lambda: device_copy(d_side[c]),
        }
        print(json.dumps({"case": c, "diffs": int(want.size), **measure(ways), "debug_device": debug[k] if debug else ""}))
    # the host form
    res = ix.compare(stream, data)
    assert res.equal and res.compared == data.size and np.array_equal(pkg.Bzip2.decompressFile(stream), data)
    ways = {
        "compare_host": lambda: ix.compare(stream, data),
        "decompress_then_array_equal": lambda: np.array_equal(pkg.Bzip2.decompressFile(stream), data),
    }
    print(json.dumps({"case": "host equal", **measure(ways), "debug_host": debug[3] if debug else ""}))
    # two streams
    res = pkg.compare_streams_device(d_in1.data_ptr(), stream1.size, ix1, d_in.data_ptr(), stream.size, ix)
    assert res.equal and res.compared == data.size and two_decodes_equal()
    ways = {
        "compare_streams_device": lambda: pkg.compare_streams_device(d_in1.data_ptr(), stream1.size, ix1, d_in.data_ptr(), stream.size, ix),
        "two_decompress_device_then_equal": two_decodes_equal,
    }
    print(json.dumps({"case": "streams level 1 / level 9", **measure(ways), "debug_streams": debug[4] if debug else ""}))


if __name__ == "__main__":
    main()
