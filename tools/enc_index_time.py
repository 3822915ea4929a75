#!/usr/bin/env python3
"""What the tables of a stream cost when the compressor hands them out, against making them afterwards, every result checked before
anything is timed.  One JSON line per group.

Input: textgen(MB x 1,000,000, seed 1) (--big: 2^30 bytes), compressed at level 9.
  device   DeviceContext.compress  |  compress_indexed(lines=False)  |  compress_indexed(lines=True)  |  the route without this
           feature: compress, the stream to the host, Bzip2Index.build, lines_build_device on the stream in HBM
  host     Bzip2.compressFile  |  compressIndexed(lines=False)  |  compressIndexed(lines=True)  |  compressFile, Bzip2Index.build,
           Bzip2Lines.build
  encoder  Bzip2Encoder, 16 MiB writes, drained after each  |  with index=True  |  with index=True, lines=True
Every repetition is a process of its own (--reps of them, one after the other, each under a time limit; the tool itself never opens
the GPU, and a child that fails or runs into its limit ends the tool).  Inside a child the ways of a group alternate, after a
warm-up of each, --inner times; the child reports each way's median.  The tool prints per way the median of the children's
medians, their spread (max - min) and all of them, and per group the surcharge of the indexed call with lines over the plain call
beside the cost of the route's two builds (route - plain).

--one-call makes one compress_indexed(lines=True) call in the device form and nothing else: the program for a kernel trace,
  rocprofv3 --kernel-trace --stats -d tool_out/enc_index_trace -- python tools/enc_index_time.py [MB] --one-call
whose stats name the time of enc_rows and enc_newlines.

usage: python tools/enc_index_time.py [MB] [--big] [--reps 3] [--inner 3]
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

PIECE = 16 << 20


def child(a, nbytes):
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    data = recipes.textgen(nbytes, 1)
    n = int(data.size)
    d_in = torch.from_numpy(np.array(data)).cuda()
    cap = n + n // 4 + 4096
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ctx = pkg.DeviceContext(0, n, 9)
    ctx.set_stage_times(False)
    ip, op = d_in.data_ptr(), d_out.data_ptr()
    if a.one_call:
        out_n, ix, ln = ctx.compress_indexed(ip, n, op, cap)
        print(json.dumps({"stream_bytes": out_n, "blocks": ix.blocks, "newlines": ln.newlines}))
        return

    def dev_route():
        out_n = ctx.compress(ip, n, op, cap)
        stream = d_out[:out_n].cpu().numpy()
        ix = pkg.Bzip2Index.build(stream)
        return out_n, ix, pkg.lines_build_device(op, out_n, ix)

    def host_route():
        s = pkg.Bzip2.compressFile(data, None, 9)
        ix = pkg.Bzip2Index.build(s)
        return s, ix, pkg.Bzip2Lines.build(s, ix)

    def encode(**kw):
        size = 0
        with pkg.Bzip2Encoder(9, 0, **kw) as enc:
            for pos in range(0, n, PIECE):
                enc.write(data[pos: pos + PIECE])
                while enc.pending:
                    size += enc.read().size
            enc.finish()
            t = enc.index() if kw else None
            while enc.pending:
                size += enc.read().size
        return size, t

    groups = {
        "device": {"compress": lambda: ctx.compress(ip, n, op, cap),
                   "compress_indexed": lambda: ctx.compress_indexed(ip, n, op, cap, lines=False),
                   "compress_indexed_lines": lambda: ctx.compress_indexed(ip, n, op, cap, lines=True),
                   "compress_then_builds": dev_route},
        "host": {"compress": lambda: pkg.Bzip2.compressFile(data, None, 9),
                 "compress_indexed": lambda: pkg.Bzip2.compressIndexed(data, 9, lines=False),
                 "compress_indexed_lines": lambda: pkg.Bzip2.compressIndexed(data, 9, lines=True),
                 "compress_then_builds": host_route},
        "encoder": {"compress": lambda: encode(), "compress_indexed": lambda: encode(index=True), "compress_indexed_lines": lambda: encode(index=True, lines=True)},
    }
    # results first: one stream, one pair of tables, whichever way made them
    _, rix, rln = dev_route()
    want_ix, want_ln = rix.save(), rln.save()
    stream = d_out[:ctx.compress(ip, n, op, cap)].cpu().numpy()
    out_n, ix, ln = ctx.compress_indexed(ip, n, op, cap)
    assert np.array_equal(d_out[:out_n].cpu().numpy(), stream) and ix.save() == want_ix and ln.save() == want_ln
    out_n, ix, none = ctx.compress_indexed(ip, n, op, cap, lines=False)
    assert none is None and ix.save() == want_ix
    s, ix, ln = pkg.Bzip2.compressIndexed(data, 9)
    assert np.array_equal(s, stream) and ix.save() == want_ix and ln.save() == want_ln
    s, ix, ln = host_route()
    assert np.array_equal(s, stream) and ix.save() == want_ix and ln.save() == want_ln
    size, (ix, ln) = encode(index=True, lines=True)
    assert size == stream.size and ix.save() == want_ix and ln.save() == want_ln
    assert encode()[0] == stream.size

    def ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rep = {"input_bytes": n, "stream_bytes": int(stream.size), "blocks": rix.blocks, "newlines": rln.newlines, "groups": {}}
    for name, ways in groups.items():
        for f in ways.values():
            f()                                             # warm-up
        ts = {w: [] for w in ways}
        for _ in range(a.inner):
            for w, f in ways.items():
                ts[w].append(ms(f))
        rep["groups"][name] = {w: round(float(np.median(v)), 3) for w, v in ts.items()}
    print(json.dumps(rep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mb", nargs="?", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=3, help="processes, one after the other")
    ap.add_argument("--inner", type=int, default=3, help="alternating runs of every way inside a process")
    ap.add_argument("--one-call", action="store_true", help="one compress_indexed call (device form, with lines) and nothing else")
    ap.add_argument("--child", action="store_true", help="(a repetition) check, time, report")
    ap.add_argument("--child-timeout", type=int, default=0, help="seconds for a repetition (default: by the input size)")
    a = ap.parse_args()
    nbytes = 1 << 30 if a.big else a.mb * 1000000
    if a.child or a.one_call:
        return child(a, nbytes)
    limit = a.child_timeout or (1500 if a.big else 120 + 4 * a.mb)
    reps = []
    for _ in range(a.reps):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(a.mb), "--child", "--inner", str(a.inner)] + (["--big"] if a.big else [])
        c = subprocess.run(cmd, capture_output=True, text=True)
        if c.returncode != 0:                               # nothing more is started on a GPU a process has just failed on
            sys.stderr.write(c.stderr[-4000:])
            sys.exit("enc_index_time: a repetition ended with status %d (124 / 137: its time limit of %d s) after %d good ones" % (c.returncode, limit, len(reps)))
        reps.append(json.loads(c.stdout.strip().splitlines()[-1]))
    print(json.dumps({k: reps[0][k] for k in ("input_bytes", "stream_bytes", "blocks", "newlines")}))
    for name in reps[0]["groups"]:
        out = {"group": name}
        med = {}
        for w in reps[0]["groups"][name]:
            v = [r["groups"][name][w] for r in reps]
            med[w] = float(np.median(v))
            out[w] = {"median_ms": round(med[w], 3), "spread_ms": round(max(v) - min(v), 3), "all_ms": v}
        out["surcharge_indexed_lines_ms"] = round(med["compress_indexed_lines"] - med["compress"], 3)
        if "compress_then_builds" in med:
            out["route_builds_ms"] = round(med["compress_then_builds"] - med["compress"], 3)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
