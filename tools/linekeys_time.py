#!/usr/bin/env python3
"""The line keys of a .bz2 stream and the line diff over them against what they ride on and what a user does without them, every
result checked before anything is timed.  One JSON line per question.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes), its index and its line table.
  keys         line_keys_device of the whole stream (stream in HBM)   against  lines_build_device (the same decode and one light
               pass over the same tiles: the yardstick) and read_ranges_device of the whole stream (the decode floor)
  diff_10 / diff_10000   diff_stream of the stream against a copy with that many lines edited, compressed at level 1 (its blocks
               fall elsewhere)   against  cjs_bzip2_decompress of both, a split into lines and the same diff over Python's hashes
               of the lines; the host time of the diff alone (diff_keys over the two key arrays) stands beside them
The ways alternate in one process after a warm-up of each: median and spread (max - min) of --reps runs (the host ways: 1 run).
The H2D / D2H bytes come from the library's "[cjs linekeys]" lines (CJS_DEBUG), collected by a child process of this tool that
makes each call once, under a time limit; if the child fails or runs into the limit, the tool stops before it opens the GPU.

--one-call makes one line_keys_device call of the whole stream and nothing else: the program for a kernel trace of its own,
  rocprofv3 --kernel-trace --stats -d tool_out/linekeys_trace -- python tools/linekeys_time.py [MB] --one-call
whose stats give the share of lk_summary / lk_chain / lk_emit in the call.

usage: python tools/linekeys_time.py [MB] [--big] [--reps 5]
"""
import argparse
import ctypes
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

N_DEBUG = 3
SEED = 0x5EED


def edited(data, nl, k):
    """the text with k of its lines replaced, evenly spread (a line longer or shorter than the one it replaces)"""
    lines = np.linspace(1, nl.size - 2, k).astype(np.int64)
    parts, at = [], 0
    for j, ln in enumerate(lines.tolist()):
        a, b = int(nl[ln - 1]) + 1, int(nl[ln]) + 1
        parts += [data[at:a], np.frombuffer(b"edited line %d of %d\n" % (j, k), dtype=np.uint8)]
        at = b
    parts.append(data[at:])
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", action="store_true", help="one line_keys_device call of the whole stream and nothing else")
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
        debug = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs linekeys]")]
        if child.returncode != 0 or len(debug) != N_DEBUG:
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("linekeys_time: the CJS_DEBUG child ended with status %d and %d of %d '[cjs linekeys]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(debug), N_DEBUG, limit))
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    L = pkg.load_library()
    data = recipes.textgen(nbytes, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    ix = pkg.Bzip2Index.build(stream)
    total = int(data.size)
    nl = np.flatnonzero(data == 10)
    d_in = torch.from_numpy(stream).cuda()
    torch.cuda.synchronize()
    ptr, n = d_in.data_ptr(), stream.size
    table = pkg.lines_build_device(ptr, n, ix)
    if a.one_call:
        keys, info = pkg.line_keys_device(ptr, n, ix, table, seed=SEED)
        print(json.dumps({"lines": int(keys.size)}))
        return

    def other(k):
        text = edited(data, nl, k)
        s = np.array(pkg.Bzip2.compressFile(text, None, 1))
        pkg.trim()
        ix_b = pkg.Bzip2Index.build(s)
        return text, s, ix_b, pkg.Bzip2Lines.build(s, ix_b)

    if a.debug_lines:
        pkg.line_keys_device(ptr, n, ix, table, seed=SEED)
        text_b, s_b, ix_b, table_b = other(10)
        ix.diff_stream(stream, table, s_b, ix_b, table_b, seed=SEED)
        return
    d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")

    def stage_keys(text):
        keys = np.zeros(int((text == 10).sum()) + 1, dtype=pkg.LINE_KEY_DTYPE)
        got = ctypes.c_size_t(0)
        L.cjs_stage_line_keys.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        assert L.cjs_stage_line_keys(text.ctypes.data, text.size, SEED, keys.ctypes.data, keys.size, ctypes.byref(got)) == 0 and got.value == keys.size
        return keys

    def host_diff(s_b, max_edits):
        sides = []
        for s in (stream, s_b):
            lines = np.asarray(pkg.Bzip2.decompressFile(s)).tobytes().split(b"\n")
            k = np.zeros(len(lines), dtype=pkg.LINE_KEY_DTYPE)
            k["hash"] = np.fromiter((hash(x) & (2 ** 60 - 1) for x in lines), dtype=np.uint64, count=len(lines))
            k["len"] = np.fromiter((len(x) & 0xFFFFFFFF for x in lines), dtype=np.uint32, count=len(lines))
            sides.append(k[:-1] if not lines[-1] else k)
        return pkg.diff_keys(sides[0], sides[1], max_edits).hunks

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    floor = lambda: pkg.read_ranges_device(ptr, n, ix, [(0, data.size)], d_full.data_ptr(), d_full.numel())
    print(json.dumps({"input_bytes": total, "stream_bytes": int(stream.size), "blocks": ix.blocks, "newlines": int(nl.size)}))
    # results first
    keys, info = pkg.line_keys_device(ptr, n, ix, table, seed=SEED)
    assert info.bad_blocks == 0 and keys.tobytes() == stage_keys(data).tobytes(), "the records differ from the host's"
    floor()
    assert np.array_equal(d_full.cpu().numpy(), data)
    groups = {"keys": {"line_keys_device": lambda: pkg.line_keys_device(ptr, n, ix, table, seed=SEED), "lines_build_device": lambda: pkg.lines_build_device(ptr, n, ix).counts(),
                       "read_ranges_device_whole": floor}}
    extra = {}
    for k in (10, 10000):
        text_b, s_b, ix_b, table_b = other(k)
        cap = 4 * k
        res = ix.diff_stream(stream, table, s_b, ix_b, table_b, max_edits=cap, seed=SEED)
        assert res.minimal and res.edits == 2 * k and res.hunks == host_diff(s_b, cap), "the diff differs from the host's"
        ka, kb = stage_keys(data), stage_keys(text_b)
        drop = lambda x: x[:-1] if x[-1]["len"] == 0 else x
        groups["diff_%d" % k] = {"diff_stream": (lambda s_b=s_b, ix_b=ix_b, table_b=table_b, cap=cap: ix.diff_stream(stream, table, s_b, ix_b, table_b, max_edits=cap, seed=SEED)),
                                 "diff_keys_alone": (lambda ka=drop(ka), kb=drop(kb), cap=cap: pkg.diff_keys(ka, kb, cap)),
                                 "decompress_both_then_host": (lambda s_b=s_b, cap=cap: host_diff(s_b, cap))}
        extra["diff_%d" % k] = {"other_stream_bytes": int(s_b.size), "other_blocks": ix_b.blocks, "hunks": len(res.hunks), "edits": res.edits}
    slow = ("decompress_both_then_host",)
    for j, (name, ways) in enumerate(groups.items()):
        for wname, f in ways.items():
            if wname not in slow:
                f()                                         # warm-up
        ts = {wname: [] for wname in ways}
        for i in range(a.reps):
            for wname, f in ways.items():
                if wname not in slow or i == 0:
                    ts[wname].append(ms(f))
        row = {"question": name, **{wname: stats(v) for wname, v in ts.items()}, **extra.get(name, {})}
        row["debug"] = debug[:1] if name == "keys" else debug[1:] if name == "diff_10" else []
        print(json.dumps(row))


if __name__ == "__main__":
    main()
