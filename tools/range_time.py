#!/usr/bin/env python3
"""Indexed range reads against the two ways to the same bytes without an index, every result checked before it is timed.  One
JSON line per case.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes) and its index (Bzip2Index.build, timed once).
  a  one 1 MiB range                      c  the whole stream as one range
  b  10,000 random ranges of 256 B        d  the ranges of b in the device form (stream and result in GPU memory)
Each against  decompress  = cjs_bzip2_decompress and a slice per range (d: decompress_device and a device slice per range), and
              blocks      = a loop of cjs_bzip2_decompress_block over the touched blocks with a host trim (a, b, c),
alternating in one process after a warm-up of each: median and spread (max - min) of --reps runs.  `pool_bytes` is what the
library's device pool holds after the case's call from an empty pool (cjs_trim before it): its scratch at the peak.  The H2D /
D2H bytes of the range calls come from the library's "[cjs range]" lines (CJS_DEBUG), collected by a child process of this tool
that makes each call once, under a time limit; if the child fails or runs into the limit, the tool stops before it opens the GPU.

usage: python tools/range_time.py [MB] [--big] [--reps 5]
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


def cases(total):
    rng = np.random.RandomState(3)
    small = [(int(o), 256) for o in rng.randint(0, total - 256, 10000)]
    return {"a": [(total // 2 + 12345, 1 << 20)], "b": small, "c": [(0, total)], "d": small}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--debug-lines", action="store_true", help="(the child) one call per case under CJS_DEBUG")
    ap.add_argument("--child-timeout", type=int, default=0, help="seconds for that child (default: by the input size)")
    a = ap.parse_args()
    nbytes = 1 << 30 if a.big else a.mb * 1000000
    debug = {}
    if not a.debug_lines:                                   # before this process opens the GPU
        # The child runs under a time limit, and anything but a clean end with its four lines stops the tool here: nothing more is
        # started on a GPU that a process has just faulted or hung on.
        limit = a.child_timeout or (1200 if a.big else 120 + 3 * a.mb)
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(a.mb), "--debug-lines"] + (["--big"] if a.big else [])
        child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, CJS_DEBUG="1"))
        lines = [ln for ln in child.stderr.splitlines() if ln.startswith("[cjs range]")]
        if child.returncode != 0 or len(lines) != 4:
            sys.stderr.write(child.stderr[-4000:])
            sys.exit("range_time: the CJS_DEBUG child ended with status %d and %d of 4 '[cjs range]' lines (124 / 137: its time limit of %d s): "
                     "nothing was timed" % (child.returncode, len(lines), limit))
        debug = dict(zip("abcd", lines))
    import torch
    import recipes
    import support
    hip = support.HipLib()                                  # (cjs_bzip2_decompress_block has no front in the package)
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()
    t0 = time.perf_counter()
    ix = pkg.Bzip2Index.build(stream)
    build_ms = (time.perf_counter() - t0) * 1e3
    entries = ix.entries()
    offs = np.concatenate([[0], np.cumsum([e[2] for e in entries])])
    d_in = torch.from_numpy(stream).cuda()
    d_full = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    d_small = torch.empty(10000 * 256, dtype=torch.uint8, device="cuda")
    C = cases(data.size)

    def ranged(name):
        if name == "d":
            off, ln, st, _ = pkg.read_ranges_device(d_in.data_ptr(), stream.size, ix, C[name], d_small.data_ptr(), d_small.numel())
            assert not st.any()
            return d_small
        buf, off, ln, st, _ = ix.read_ranges_raw(stream, C[name])
        assert not st.any()
        return buf

    def by_decompress(name):
        if name == "d":
            pkg.decompress_device(d_in.data_ptr(), stream.size, d_full.data_ptr(), d_full.numel())
            return torch.cat([d_full[o:o + n] for o, n in C[name]])
        out = pkg.Bzip2.decompressFile(stream)
        return out if name == "c" else np.concatenate([out[o:o + n] for o, n in C[name]])

    def by_blocks(name):
        touched = sorted({b for o, n in C[name] for b in range(int(np.searchsorted(offs, o, "right")) - 1, int(np.searchsorted(offs, o + n - 1, "right")))})
        dec = {b: hip.bzip2_decompress_block(stream, entries[b][0])[1] for b in touched}
        parts = []
        for o, n in C[name]:
            for b in range(int(np.searchsorted(offs, o, "right")) - 1, int(np.searchsorted(offs, o + n - 1, "right"))):
                lo, hi = max(o, int(offs[b])), min(o + n, int(offs[b + 1]))
                parts.append(dec[b][lo - int(offs[b]):hi - int(offs[b])])
        return np.concatenate(parts)

    if a.debug_lines:
        for name in "abcd":
            ranged(name)
        return

    def ms(f, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f(name)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    print(json.dumps({"input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": len(entries), "index_build_ms": round(build_ms, 2),
                      "index_bytes": len(ix.save())}))
    for name in "abcd":
        want = np.concatenate([data[o:o + n] for o, n in C[name]])
        ways = {"ranges": ranged, "decompress": by_decompress}
        if name != "d":
            ways["blocks"] = by_blocks
        pool = {}
        for k, f in ways.items():                           # results first, each from an empty pool
            pkg.trim()
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            got = f(name)
            torch.cuda.synchronize()
            pool[k] = int(free0 - torch.cuda.mem_get_info()[0])
            got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
            assert np.array_equal(got, want), (name, k)
            del got
        reps = {k: (min(a.reps, 2) if k == "blocks" and len(entries) > 200 else a.reps) for k in ways}
        ts = {k: [] for k in ways}
        for i in range(a.reps):                             # (the checked run above was each way's warm-up)
            for k, f in ways.items():
                if i < reps[k]:
                    ts[k].append(ms(f, name)[0])
        print(json.dumps({"case": name, "ranges": len(C[name]), "bytes": int(want.size), **{k: stats(v) for k, v in ts.items()},
                          "pool_bytes": pool, "debug": debug.get(name, "")}))


if __name__ == "__main__":
    main()
