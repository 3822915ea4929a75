#!/usr/bin/env python3
"""Recovery timing against decompression, every result checked before it is timed.  One JSON line per measurement.

Input: the level-9 stream of textgen(MB x 1,000,000, seed 1), undamaged -- so recovery has to give what decompression gives.
  host    cjs_bzip2_recover (bytes form, stream form) against cjs_bzip2_decompress, alternating in one process after a warm-up of
          each: median and spread (max - min) of --reps runs each
  device  recover_device (both forms) against decompress_device, the same way, and one device copy of the output for scale
  --profile decompress|recover: three calls of cjs_bzip2_decompress, or of the bytes form, and nothing else (for a kernel trace
          of its own; the compressor's kernels in front of them have other names)

usage: python tools/recover_time.py [MB] [--reps 7] [--profile decompress|recover]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile", choices=("decompress", "recover"))
    a = ap.parse_args()
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(a.mb * 1000000, 1)
    stream = np.array(pkg.Bzip2.compressFile(data, None, 9))
    pkg.trim()

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ts):
        return {"median_ms": round(float(np.median(ts)), 3), "spread_ms": round(float(max(ts) - min(ts)), 3), "all_ms": [round(t, 2) for t in ts]}

    if a.profile:
        for _ in range(3):
            out = pkg.Bzip2.decompressFile(stream) if a.profile == "decompress" else pkg.Bzip2.recoverFile(stream)[0]
            assert np.array_equal(out, data)
        print(json.dumps({"profile": a.profile, "calls": 3}))
        return
    # results first
    got, found = pkg.Bzip2.recoverFile(stream)
    assert np.array_equal(got, data) and all(f[4] == 0 for f in found)
    rep, _ = pkg.Bzip2.recoverFile(stream, None, True)
    assert np.array_equal(rep, stream)                              # a level-9 single stream is its own repair
    assert np.array_equal(pkg.Bzip2.decompressFile(stream), data)
    del got, rep
    host = {"decompress": lambda: pkg.Bzip2.decompressFile(stream), "recover_bytes": lambda: pkg.Bzip2.recoverFile(stream),
            "recover_stream": lambda: pkg.Bzip2.recoverFile(stream, None, True)}
    ts = {k: [] for k in host}
    for i in range(a.reps + 1):
        for k, f in host.items():
            t, _ = ms(f)
            if i:                                                   # (run 0 of each is its warm-up)
                ts[k].append(t)
    print(json.dumps({"part": "host", "input_bytes": int(data.size), "stream_bytes": int(stream.size), "blocks": len(found), **{k: stats(v) for k, v in ts.items()}}))

    d_in = torch.from_numpy(stream).cuda()
    d_out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    d_ref = torch.from_numpy(data).cuda()
    d_cp = torch.empty_like(d_out)
    dev = {"decompress_device": lambda: pkg.decompress_device(d_in.data_ptr(), stream.size, d_out.data_ptr(), d_out.numel()),
           "recover_device_bytes": lambda: pkg.recover_device(d_in.data_ptr(), stream.size, d_out.data_ptr(), d_out.numel())[0],
           "recover_device_stream": lambda: pkg.recover_device(d_in.data_ptr(), stream.size, d_out.data_ptr(), d_out.numel(), True)[0],
           "device_copy_of_output": lambda: d_cp.copy_(d_ref)}
    for k in ("decompress_device", "recover_device_bytes"):
        d_out.zero_()
        assert dev[k]() == data.size and torch.equal(d_out, d_ref), k
    assert dev["recover_device_stream"]() == stream.size and torch.equal(d_out[: stream.size], d_in)
    ts = {k: [] for k in dev}
    for i in range(a.reps + 1):
        for k, f in dev.items():
            t, _ = ms(f)
            if i:
                ts[k].append(t)
    print(json.dumps({"part": "device", "input_bytes": int(data.size), **{k: stats(v) for k, v in ts.items()}}))


if __name__ == "__main__":
    main()
