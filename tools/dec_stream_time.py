"""Streaming decoder timing: one-shot cjs_bzip2_decompress against the streaming decoder (cjs_bzip2_dec_*) fed from host memory, on
the level-9 streams of tools/textgen.c text: textgen(1e8, seed 1) and 2^30 bytes.  Both outputs are checked first (sha256 of the
text), then the two paths are timed in alternation (wall clock, the whole call: upload, kernels, download); the median and the
spread (min .. max) of each are printed as one JSON line per (input, chunk, out).

usage: python tools/dec_stream_time.py [--sizes 100000000,1073741824] [--chunks-mib 0,16,64,256] [--out-mib 0,64,256,1024] [--reps 5]
       (0 = the library's default)
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


def stream_once(pkg, stream, chunk, out_bytes, write_piece, sink):
    """the whole stream through a decoder, drained after every write; sink(piece) sees the output in order"""
    with pkg.Bzip2Decoder(False, chunk, out_bytes) as dec:
        def drain():
            while True:
                p = dec.read(16 << 20)
                if not p.size:
                    return
                sink(p)
        for pos in range(0, stream.size, write_piece):
            piece = stream[pos: pos + write_piece]
            while piece.size:
                piece = piece[dec.write(piece):]
                drain()
        dec.finish()
        drain()
        assert dec.done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000000,1073741824")
    ap.add_argument("--chunks-mib", default="0,16,64,256")
    ap.add_argument("--out-mib", default="0,64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--write-mib", type=int, default=16, help="size of one write() call")
    a = ap.parse_args()
    import recipes
    pkg = importlib.import_module("compressjs-flattened_amd")
    for n in (int(x) for x in a.sizes.split(",")):
        data = recipes.textgen(n, 1)
        want = hashlib.sha256(data.tobytes()).hexdigest()
        stream = pkg.Bzip2.compressFile(data, None, a.level).copy()
        del data
        one = pkg.Bzip2.decompressFile(stream)
        if one.size != n or hashlib.sha256(one.tobytes()).hexdigest() != want:
            raise SystemExit("one-shot result of %d bytes differs from the text" % n)
        del one
        for chunk_mib in (int(x) for x in a.chunks_mib.split(",")):
            for out_mib in (int(x) for x in a.out_mib.split(",")):
                chunk, out_bytes = chunk_mib << 20, out_mib << 20
                h = hashlib.sha256()
                stream_once(pkg, stream, chunk, out_bytes, a.write_mib << 20, lambda p: h.update(p.tobytes()))
                if h.hexdigest() != want:
                    raise SystemExit("streamed result of %d bytes (chunk %d MiB, out %d MiB) differs from the text" % (n, chunk_mib, out_mib))
                t_one, t_str = [], []
                for _ in range(a.reps):                      # alternating: both see the same state of the box
                    t0 = time.perf_counter()
                    r = pkg.Bzip2.decompressFile(stream)
                    t_one.append(time.perf_counter() - t0)
                    del r
                    got = [0]

                    def count(p):
                        got[0] += p.size
                    t0 = time.perf_counter()
                    stream_once(pkg, stream, chunk, out_bytes, a.write_mib << 20, count)
                    t_str.append(time.perf_counter() - t0)
                    assert got[0] == n
                med1, med2 = statistics.median(t_one), statistics.median(t_str)
                print(json.dumps({"bytes_out": n, "level": a.level, "chunk_mib": chunk_mib, "out_mib": out_mib, "reps": a.reps, "bytes_in": int(stream.size),
                                  "one_shot_ms": [round(x * 1e3, 1) for x in (min(t_one), med1, max(t_one))],
                                  "stream_ms": [round(x * 1e3, 1) for x in (min(t_str), med2, max(t_str))],
                                  "one_shot_MB_per_s": round(n / med1 / 1e6, 1), "stream_MB_per_s": round(n / med2 / 1e6, 1),
                                  "stream_over_one_shot": round(med2 / med1, 3)}), flush=True)


if __name__ == "__main__":
    main()
