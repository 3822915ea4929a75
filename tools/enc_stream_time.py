"""Streaming encoder timing: one-shot cjs_bzip2_compress against the streaming encoder (cjs_bzip2_enc_*) fed from host memory, on
tools/textgen.c text: textgen(1e8, seed 1) and 2^30 bytes.  Both outputs are checked against the golden first (sha256), then
the two paths are timed in alternation (wall clock, the whole call: upload, kernels, download); the median and the spread
(min .. max) of each are printed as one JSON line per (input, chunk).

usage: python tools/enc_stream_time.py [--sizes 100000000,1073741824] [--chunks-mib 0,32,64,128,256] [--reps 5] [--level 9]
       (chunk 0 = the library's default)
"""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = {(100000000, 9): "golden_big_bzip2_9_100m.json", (1 << 30, 9): "golden_big_bzip2_9_1g.json",
          (100000000, 1): "golden_big_bzip2_1_100m.json"}


def stream_once(pkg, data, level, chunk, write_piece, sink):
    """the whole input through an encoder, drained after every write; sink(piece) sees the output in order"""
    with pkg.Bzip2Encoder(level, chunk) as enc:
        for pos in range(0, data.size, write_piece):
            enc.write(data[pos: pos + write_piece])
            while enc.pending:
                sink(enc.read(8 << 20))
        enc.finish()
        while enc.pending:
            sink(enc.read(8 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000000,1073741824")
    ap.add_argument("--chunks-mib", default="0,32,64,128,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--write-mib", type=int, default=16, help="size of one write() call")
    a = ap.parse_args()
    import recipes
    import support
    pkg = importlib.import_module("compressjs-flattened_amd")
    for n in (int(x) for x in a.sizes.split(",")):
        data = recipes.textgen(n, 1)
        name = GOLDEN.get((n, a.level))
        want = support.load_golden(name)["cases"][0]["out_sha256"] if name else None
        one = pkg.Bzip2.compressFile(data, None, a.level)
        one_sha = support.sha256(one)
        if want and one_sha != want:
            raise SystemExit("one-shot stream of %d bytes differs from the golden" % n)
        out_len = int(one.size)
        del one
        for chunk_mib in (int(x) for x in a.chunks_mib.split(",")):
            chunk = chunk_mib << 20
            h = hashlib.sha256()
            stream_once(pkg, data, a.level, chunk, a.write_mib << 20, lambda p: h.update(p.tobytes()))
            if h.hexdigest() != (want or one_sha):
                raise SystemExit("streamed output of %d bytes (chunk %d MiB) differs from the %s" % (n, chunk_mib, "golden" if want else "one-shot stream"))
            t_one, t_str = [], []
            for _ in range(a.reps):                      # alternating: both see the same state of the box
                t0 = time.perf_counter()
                r = pkg.Bzip2.compressFile(data, None, a.level)
                t_one.append(time.perf_counter() - t0)
                del r
                got = [0]

                def count(p):
                    got[0] += p.size
                t0 = time.perf_counter()
                stream_once(pkg, data, a.level, chunk, a.write_mib << 20, count)
                t_str.append(time.perf_counter() - t0)
                assert got[0] == out_len
            med1, med2 = statistics.median(t_one), statistics.median(t_str)
            print(json.dumps({"bytes_in": n, "level": a.level, "chunk_mib": chunk_mib, "reps": a.reps, "bytes_out": out_len,
                              "one_shot_ms": [round(x * 1e3, 1) for x in (min(t_one), med1, max(t_one))],
                              "stream_ms": [round(x * 1e3, 1) for x in (min(t_str), med2, max(t_str))],
                              "one_shot_MB_per_s": round(n / med1 / 1e6, 1), "stream_MB_per_s": round(n / med2 / 1e6, 1),
                              "stream_over_one_shot": round(med2 / med1, 3)}), flush=True)


if __name__ == "__main__":
    main()
