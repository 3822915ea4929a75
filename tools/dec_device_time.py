"""Device-resident decompress timing, every result checked before it is timed.  Prints one JSON line per measurement.

  single  decompress_device vs the host-buffer cjs_bzip2_decompress of the same stream, alternating, --reps runs each; the host
          path's spread against itself (max - min of its runs) is the margin.  Inputs: textgen(100,000,000, seed 1) at level 9
          (the bench input) and, with --big, the 2^30-byte golden.
  batch   decompress_batch_device vs cjs_bzip2_decompress_batch vs a loop of decompress_device over the same streams (the workloads
          of tools/batch_dec_time.py), best of --breps.
  trip    device compress -> device decompress of the 100 MB input: no host copy of either stream.

usage: python tools/dec_device_time.py [--reps 7] [--breps 3] [--big] [--parts single,batch,trip] [--workloads 20000x1-300,4096x65536,1024x900000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
u8p = ctypes.POINTER(ctypes.c_uint8)
S = ctypes.c_size_t


def _ms(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def single(pkg, L, name, data, stream, reps):
    import torch
    d_in = torch.from_numpy(stream).cuda()
    d_out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    ref = torch.from_numpy(data).cuda()
    sp = stream.ctypes.data_as(u8p)

    def host():
        out, n = u8p(), S(0)
        rc = L.cjs_bzip2_decompress(sp, stream.size, 0, ctypes.byref(out), ctypes.byref(n), None)
        assert rc == 0 and n.value == data.size
        return out

    def dev():
        assert pkg.decompress_device(d_in.data_ptr(), stream.size, d_out.data_ptr(), d_out.numel()) == data.size

    out = host()                                                     # checked (and warm) first
    assert np.array_equal(np.ctypeslib.as_array(out, (data.size,)), data)
    L.cjs_free(out)
    dev()
    assert torch.equal(d_out, ref)
    th, td = [], []
    for _ in range(reps):
        th.append(_ms(lambda: L.cjs_free(host())))
        td.append(_ms(dev))
    print(json.dumps({"part": "single", "input": name, "bytes_out": int(data.size), "bytes_in": int(stream.size), "reps": reps,
                      "host_ms_median": round(float(np.median(th)), 2), "device_ms_median": round(float(np.median(td)), 2),
                      "host_spread_ms": round(max(th) - min(th), 2), "host_ms": [round(x, 2) for x in th], "device_ms": [round(x, 2) for x in td]}), flush=True)


def batch(pkg, L, wl, level, breps):
    import torch
    import recipes
    count, sz = wl.split("x")
    count = int(count)
    lo, hi = (int(x) for x in (sz.split("-") if "-" in sz else (sz, sz)))
    sizes = np.random.default_rng(5).integers(lo, hi + 1, count)
    xs = [recipes.textgen(int(n), 1000 + k) for k, n in enumerate(sizes)]
    ss = [np.ascontiguousarray(s) for s in pkg.Bzip2.compressFiles(xs, level)]
    total = sum(int(x.size) for x in xs)
    offs = np.concatenate([[0], np.cumsum([s.size for s in ss])]).astype(np.uint64)
    d_in = torch.from_numpy(np.concatenate(ss)).cuda()
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    ref = torch.from_numpy(np.concatenate(xs)).cuda()
    ptrs = (u8p * count)(*[s.ctypes.data_as(u8p) for s in ss])
    lens = (S * count)(*[s.size for s in ss])
    off, ln, st = (S * count)(), (S * count)(), (ctypes.c_int32 * count)()

    def host_batch():
        out = u8p()
        assert L.cjs_bzip2_decompress_batch(ptrs, lens, count, 0, ctypes.byref(out), off, ln, st, None) == 0
        L.cjs_free(out)

    def dev_batch():
        o, n, s, _ = pkg.decompress_batch_device(d_in.data_ptr(), offs, d_out.data_ptr(), total)
        assert not s.any()

    def dev_loop():
        at = 0
        for k in range(count):
            at += pkg.decompress_device(d_in.data_ptr() + int(offs[k]), int(offs[k + 1] - offs[k]), d_out.data_ptr() + at, total - at)

    dev_batch()
    assert torch.equal(d_out, ref)
    d_out.zero_()
    dev_loop()
    assert torch.equal(d_out, ref)
    tb = min(_ms(dev_batch) for _ in range(breps))
    th = min(_ms(host_batch) for _ in range(breps))
    tl = _ms(dev_loop)
    print(json.dumps({"part": "batch", "workload": wl, "level": level, "count": count, "bytes_out": total, "bytes_in": int(offs[-1]),
                      "device_batch_ms": round(tb, 2), "host_batch_ms": round(th, 2), "device_loop_ms": round(tl, 2)}), flush=True)


def trip(pkg, data):
    import torch
    d_in = torch.from_numpy(data).cuda()
    d_s = torch.empty(data.size // 2 + (1 << 20), dtype=torch.uint8, device="cuda")
    d_out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    ctx = pkg.DeviceContext(0, data.size, 9)
    m = [0]

    def comp():
        m[0] = ctx.compress(d_in.data_ptr(), data.size, d_s.data_ptr(), d_s.numel())

    def dec():
        assert pkg.decompress_device(d_s.data_ptr(), m[0], d_out.data_ptr(), d_out.numel()) == data.size
    comp(); dec()
    assert torch.equal(d_out, d_in)
    tc = [_ms(comp) for _ in range(3)]
    td = [_ms(dec) for _ in range(3)]
    ctx.close()
    print(json.dumps({"part": "trip", "bytes": int(data.size), "stream": m[0], "compress_ms_median": round(float(np.median(tc)), 2),
                      "decompress_ms_median": round(float(np.median(td)), 2), "round_trip": True}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--breps", type=int, default=3)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--parts", default="single,batch,trip")
    ap.add_argument("--workloads", default="20000x1-300,4096x65536,1024x900000")
    a = ap.parse_args()
    import importlib
    import recipes
    import support
    pkg = importlib.import_module("compressjs-flattened_amd")
    L = pkg.load_library()
    parts = a.parts.split(",")
    data = recipes.textgen(100000000, 1)
    if "single" in parts:
        single(pkg, L, "textgen 1e8 s1 level 9", data, np.ascontiguousarray(pkg.Bzip2.compressFile(data, None, 9)), a.reps)
        if a.big:
            g = support.load_golden("golden_big_bzip2_9_1g.json")["cases"][0]
            big = recipes.build(g["recipe"])
            single(pkg, L, "golden 2^30 level 9", big, np.ascontiguousarray(pkg.Bzip2.compressFile(big, None, 9)), a.reps)
            del big
    if "batch" in parts:
        for wl in a.workloads.split(","):
            for level in (9, 1):
                batch(pkg, L, wl, level, a.breps)
    if "trip" in parts:
        trip(pkg, data)


if __name__ == "__main__":
    main()
