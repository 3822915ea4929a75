"""Batch path timing: N inputs of tools/textgen.c text (COUNTxSIZE, or COUNTxMIN-MAX for random sizes) (distinct seeds), device-resident, compressed as ONE batch
(cjs_bzip2_compress_batch_device) and as a loop of single-stream calls (cjs_bzip2_compress_device) in the same process.
Every batch stream is checked against the single-call stream before the timed loops.  Prints one JSON line per workload.

usage: python tools/batch_time.py [--reps R] [--workloads 4096x65536,1024x900000,20000x1-300] [--levels 9,1]
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="4096x65536,1024x900000,20000x1-300")
    ap.add_argument("--levels", default="9,1")
    a = ap.parse_args()
    import importlib
    import torch
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    dev = torch.device("cuda:0")
    for wl in a.workloads.split(","):
        count, sz = wl.split("x")
        count = int(count)
        lo, hi = (int(x) for x in (sz.split("-") if "-" in sz else (sz, sz)))     # COUNTxSIZE or COUNTxMIN-MAX (random sizes)
        sizes = np.random.default_rng(5).integers(lo, hi + 1, count)
        ins = [recipes.textgen(int(n), 1000 + k) for k, n in enumerate(sizes)]
        size = hi
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([d.size for d in ins])
        total_in = int(off[-1])
        d_in = torch.from_numpy(np.concatenate(ins)).to(dev)
        d_out = torch.zeros(total_in + total_in // 4 + 65536 * count // 64 + (1 << 20), dtype=torch.uint8, device=dev)
        d_one = torch.zeros(size + size // 4 + 4096, dtype=torch.uint8, device=dev)
        for level in (int(x) for x in a.levels.split(",")):
            bctx = pkg.DeviceContext.batch(0, total_in, count, level)
            sctx = pkg.DeviceContext(0, size, level)
            # correctness first: every batch stream equals the single-call stream
            so, sl = bctx.compress_batch(d_in.data_ptr(), off, d_out.data_ptr(), d_out.numel())
            host = d_out.cpu().numpy()
            for k in range(count):
                n = sctx.compress(d_in.data_ptr() + int(off[k]), int(off[k + 1] - off[k]), d_one.data_ptr(), d_one.numel())
                if not np.array_equal(host[int(so[k]): int(so[k] + sl[k])], d_one[:n].cpu().numpy()):
                    raise SystemExit("batch stream %d differs from the single-call stream" % k)
            torch.cuda.synchronize()
            t_batch = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                bctx.compress_batch(d_in.data_ptr(), off, d_out.data_ptr(), d_out.numel())
                t_batch.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for k in range(count):
                sctx.compress(d_in.data_ptr() + int(off[k]), int(off[k + 1] - off[k]), d_one.data_ptr(), d_one.numel())
            t_loop = time.perf_counter() - t0
            tb = min(t_batch)
            print(json.dumps({"workload": wl, "level": level, "bytes_in": total_in, "bytes_out": int(sl.sum()),
                              "batch_ms": round(tb * 1e3, 2), "batch_items_per_s": round(count / tb, 1),
                              "batch_MB_per_s": round(total_in / tb / 1e6, 1), "loop_ms": round(t_loop * 1e3, 2),
                              "loop_MB_per_s": round(total_in / t_loop / 1e6, 1), "speedup": round(t_loop / tb, 2)}), flush=True)
            bctx.close()
            sctx.close()


if __name__ == "__main__":
    main()
