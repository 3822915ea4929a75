"""Batch decompress timing: N streams made by Bzip2.compressFiles of tools/textgen.c text (COUNTxSIZE, or COUNTxMIN-MAX for
random sizes; distinct seeds), decoded as ONE cjs_bzip2_decompress_batch call and as a loop of cjs_bzip2_decompress calls
over the same streams, in the same process.  Every output is checked against its input before the timed runs.  Prints one
JSON line per workload and level.

usage: python tools/batch_dec_time.py [--reps R] [--loop-reps R] [--workloads 20000x1-300,4096x65536,1024x900000] [--levels 9,1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--workloads", default="20000x1-300,4096x65536,1024x900000")
    ap.add_argument("--levels", default="9,1")
    a = ap.parse_args()
    import importlib
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    L = pkg.load_library()
    for wl in a.workloads.split(","):
        count, sz = wl.split("x")
        count = int(count)
        lo, hi = (int(x) for x in (sz.split("-") if "-" in sz else (sz, sz)))
        sizes = np.random.default_rng(5).integers(lo, hi + 1, count)
        xs = [recipes.textgen(int(n), 1000 + k) for k, n in enumerate(sizes)]
        total_out = sum(int(x.size) for x in xs)
        for level in (int(v) for v in a.levels.split(",")):
            ss = [np.ascontiguousarray(s) for s in pkg.Bzip2.compressFiles(xs, level)]
            ptrs = (u8p * count)(*[s.ctypes.data_as(u8p) for s in ss])
            lens = (S * count)(*[s.size for s in ss])
            off, ln, st = (S * count)(), (S * count)(), (ctypes.c_int32 * count)()

            def run_batch():
                out = u8p()
                rc = L.cjs_bzip2_decompress_batch(ptrs, lens, count, 0, ctypes.byref(out), off, ln, st, None)
                if rc:
                    raise SystemExit("batch call failed: %d" % rc)
                return out

            def run_loop(check):
                for k in range(count):
                    out, n = u8p(), S(0)
                    rc = L.cjs_bzip2_decompress(ptrs[k], lens[k], 0, ctypes.byref(out), ctypes.byref(n), None)
                    if rc:
                        raise SystemExit("single call %d failed: %d" % (k, rc))
                    if check and (n.value != xs[k].size or ctypes.string_at(out, n.value) != xs[k].tobytes()):
                        raise SystemExit("single call %d differs from its input" % k)
                    L.cjs_free(out)

            out = run_batch()                                        # correctness first (and warm-up)
            base = ctypes.addressof(out.contents)
            for k in range(count):
                if st[k] or ln[k] != xs[k].size or ctypes.string_at(base + off[k], ln[k]) != xs[k].tobytes():
                    raise SystemExit("batch output %d differs from its input" % k)
            L.cjs_free(out)
            run_loop(True)
            t_batch = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                L.cjs_free(run_batch())
                t_batch.append(time.perf_counter() - t0)
            t_loop = []
            for _ in range(a.loop_reps):
                t0 = time.perf_counter()
                run_loop(False)
                t_loop.append(time.perf_counter() - t0)
            tb, tl = min(t_batch), min(t_loop)
            print(json.dumps({"workload": wl, "level": level, "count": count, "bytes_out": total_out,
                              "bytes_in": int(sum(s.size for s in ss)), "batch_ms": round(tb * 1e3, 2), "loop_ms": round(tl * 1e3, 2),
                              "batch_MBps": round(total_out / tb / 1e6, 1), "loop_MBps": round(total_out / tl / 1e6, 1),
                              "speedup": round(tl / tb, 2)}), flush=True)


if __name__ == "__main__":
    main()
